"""The stamps of the bit-identity record of the convolution stage (tests/golden/conv_stamps_gfx950.npz), shared by
scripts/record_conv_stamps.py, which writes the record, and tests/test_gpu_conv_bits.py, which holds a build to it.

Context.convolve_stamps (k_conv_fft<float, double> in the mixed mode, k_conv_fft<double, double> in the f64 mode) on a
dim = 128 context at grid_pixscale(512): the two tasks of tests/test_gpu_conv.py, whose tip-tilt kernels differ
six-fold in width, at 465 and 930 nm, each on two classes of input -- eight stamps per mode, one call:

  moffat  an off-centre Moffat-like stamp, its peak at a different pixel in each of the four stamps, with a seeded
          ripple of 1e-3 of the peak on top;
  hard    unit impulses at (0, 0), (0, 39), (39, 0), (39, 39) and (20, 21) on the 0 / 1 checkerboard
          (1 + (-1)^(i + j)) / 2: its energy sits in the DC and Nyquist column and row of the 64 x 64 frame, which is what
          slot 0 of the kernel carries as one packed column.

Both classes fill every row pair and every column, so every slot, the zero-padded rows 40-63 and the packed column are
exercised.  Only generation parameters are kept: the Moffats use exponents 2 and 2.5, for which the profile is a few
multiplications, a square root and a division -- operations IEEE 754 rounds exactly -- and the generator's doubles are
the same on every machine; the record holds the SHA-256 of the inputs, and the test compares that first.

The record keeps the mixed outputs as float32 (they are float values) and the f64 outputs as float64, each as the byte
planes of its little-endian values (planes / values below: byte b of every value, then byte b + 1 of every value):
sign and exponent bytes then lie together and deflate takes them away, 117 KB where the arrays as they stand take 140.
"""
import hashlib
import os

import numpy as np

NS = 40
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
RECORD = os.path.join(GOLDEN, 'conv_stamps_gfx950.npz')
MODES = ('mixed', 'f64')
DTYPE = {'mixed': np.float32, 'f64': np.float64}
DIM = 128
GRID = 512                                     # the context's pixel scale is grid_pixscale(GRID)
LBDA = np.array([465.0, 930.0])
TASKS = np.array([(0.6, 0.9, 25.0), (2.0, 0.1, 10.0)])      # (seeing, GL, L0): those of tests/test_gpu_conv.py
CLASSES = ('moffat', 'hard')
SEED = 512
IMPULSES = ((0, 0), (0, 39), (39, 0), (39, 39), (20, 21))


def moffat_like(peak, p0, q0, a2, n, ripple):
    p, q = np.mgrid[:NS, :NS].astype(np.float64)
    g = 1.0 + ((p - p0) * (p - p0) + (q - q0) * (q - q0)) / a2
    den = {2.0: g * g, 2.5: g * g * np.sqrt(g)}[n]
    return peak / den + (1e-3 * peak) * ripple


def hard():
    i, j = np.indices((NS, NS))
    s = np.where((i + j) % 2 == 0, 1.0, 0.0)
    for a, b in IMPULSES:
        s[a, b] += 1.0
    return s


def inputs():
    """(pre, par): pre (4, 2, 40, 40) float64, task 2 c + k is class c with the parameters of TASKS[k]; par (4, 3)"""
    rng = np.random.default_rng(SEED)
    pre = np.empty((2 * len(TASKS), LBDA.size, NS, NS))
    peaks = set()
    for k in range(len(TASKS)):
        for l in range(LBDA.size):
            m = 2 * k + l
            p0, q0 = (13, 26, 22, 17)[m] + 0.25 * (m - 1), (24, 15, 19, 27)[m] - 0.25 * m
            s = moffat_like(rng.uniform(0.5, 2.0), p0, q0, rng.uniform(3.0, 30.0), (2.0, 2.5)[m % 2], rng.random((NS, NS)))
            peaks.add(int(np.argmax(s)))
            pre[k, l] = s
            pre[len(TASKS) + k, l] = hard()
    assert len(peaks) == 4 and np.all(pre[:len(TASKS)] > 0)
    return pre, np.tile(TASKS, (len(CLASSES), 1))


def digest(pre):
    return hashlib.sha256(np.ascontiguousarray(pre, dtype='<f8').tobytes()).hexdigest()


def planes(a, prec):
    """(itemsize, a.size) uint8: the values of `a` in the record's type of the mode, byte plane by byte plane"""
    v = np.ascontiguousarray(a, dtype=np.dtype(DTYPE[prec]).newbyteorder('<'))
    return np.ascontiguousarray(v.reshape(-1).view(np.uint8).reshape(v.size, v.itemsize).T)


def values(p, prec, shape):
    """the array `planes` made its argument from"""
    dt = np.dtype(DTYPE[prec]).newbyteorder('<')
    assert p.dtype == np.uint8 and p.shape == (dt.itemsize, int(np.prod(shape)))
    return np.ascontiguousarray(p.T).view(dt).reshape(shape).astype(DTYPE[prec])


def record(api, precisions=MODES):
    """The outputs of the library `api` loads: {'out_<mode>': (4, 2, 40, 40) float64}"""
    pre, par = inputs()
    out = {}
    for prec in precisions:
        ctx = api.Context(dim=DIM, pixscale=api.grid_pixscale(GRID), precision=prec)
        out['out_%s' % prec] = ctx.convolve_stamps(LBDA, par[:, 0], par[:, 1], par[:, 2], pre)
        ctx.close()
    return out
