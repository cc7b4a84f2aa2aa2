// Where the arrays of one stamp, frame or cube call lie in the context's staging buffer ("The entry layer").
// Plain arithmetic without HIP, so that it compiles and is checked on the CPU alone (tests/test_stage_layout_host.py).
#pragma once

#include <cassert>
#include <cstddef>

namespace mpsfr {
namespace host {

// The arrays are declared in the order of the call; place() puts the inputs of 8-byte elements first, in that order,
// then the outputs, each padded to 8 bytes, then the narrower inputs (int32 indices), so that everything is aligned.
// An absent optional array gets no room.
struct StageLayout {
    static constexpr int kMaxArrays = 14;      // 8 inputs and 6 outputs: the widest call (mpsfr_fit_cube_psf_free)
    struct Array { size_t bytes, elem, offset; bool output, present; };
    Array a[kMaxArrays];
    int n = 0;

    // -> the index of the array in `a`
    int add(bool present, size_t count, size_t elem, bool output) {
        assert(n < kMaxArrays);
        a[n] = {count * elem, elem, 0, output, present};
        return n++;
    }

    // sets every present array's offset -> the bytes they take together
    size_t place() {
        size_t bytes = 0;
        for (int pass = 0; pass < 3; ++pass)
            for (int k = 0; k < n; ++k) {
                const int group = a[k].output ? 1 : a[k].elem < 8 ? 2 : 0;
                if (!a[k].present || group != pass) continue;
                a[k].offset = bytes;
                bytes += a[k].output ? (a[k].bytes + 7) & ~(size_t)7 : a[k].bytes;
            }
        return bytes;
    }
};

}  // namespace host
}  // namespace mpsfr
