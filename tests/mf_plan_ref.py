"""The work plan of the per-wavelength stage in NumPy (float64).  TEST INFRASTRUCTURE.

The per-wavelength stage runs the part of the OTF half plane a plan selects: block masks in three tiers, the k-step and
sweep words derived from them and the work items of k_otf_mfma2 (k_mf_prep), the lines kept per wavelength pair and the
task order of the other forms (k_vkeep, k_task_order), the floor per task of the kernel for several directions
(k_peak_floor), all from minima of the stored structure function (k_dmin).  Two layers, from DESIGN.md 2.9 and
include/mpsfr.h:

(R) the rule: what those kernels are meant to decide, from the inputs they read (`Context.debug_fetch`), every sum in
    float64; `compare_plan` / `compare_vkeep` say where a fetched plan differs from it;
(G) the guarantee: what the header promises about the plan, whichever way it was reached -- the true OTF mass of what
    a plan leaves out, from `dphi0` and `tel` alone, against prune_eps and tier_eps.  No tolerance: the bounds the
    kernels use are upper bounds by construction.

Planes are the library's transposed half planes: [dim/2+1 lines v][dim columns u]; a block is 16 lines x 32 columns
(m-tile mt, k-step ks), a sweep eight m-tiles.  Mask words hold bit ks.
"""
import collections

import numpy as np

MTL, KBL, KT2, NLISTS = 16, 32, 8, 64
LOG2E = np.float32(1.44269504088896340736)
F32 = np.float32

# The rungs of tier_eps the tests walk: the default, then down to where the floor threshold is clamped at the eps
# threshold and no mid block is left (tests/test_mf_plan_ref.py shows what they reach on the oracle's planes).
LADDER = (4e-6, 1e-7, 1e-8, 1e-9, 1e-10, 1e-12)

Par = collections.namedtuple('Par', 'thr_eps thr_floor thr_mid tier_half thr_blk thr_sum c2min per ngr c')


def parse_par(v):
    """debug fetch `mf_par` [9 + nl] -> Par (the thresholds as the float32 values the kernels got)."""
    v = np.asarray(v, dtype=np.float64)
    return Par(*[F32(x) for x in v[:7]], int(v[7]), int(v[8]), v[9:].copy())


def geometry(dim):
    """H1 lines, nks k-steps, nmt m-tiles, nsw sweeps of a grid."""
    h1 = dim // 2 + 1
    nmt = (h1 + MTL - 1) // MTL
    return h1, dim // KBL, nmt, (nmt + KT2 - 1) // KT2


def peak_lines(dim):
    return 2 if dim > 512 else 4


def groups(nl, permax=6):
    """(per, ngr): wavelength groups of at most `permax`, as even as possible."""
    permax = min(permax, 7)
    ngr = (nl + permax - 1) // permax
    return (nl + ngr - 1) // ngr, ngr


def c2_of(c):
    """float32(float32(c) float32(log2 e)): the exponent factor of a wavelength as the kernels form it."""
    return F32(F32(c) * LOG2E)


def host_par(dim, lbda_nm, ndb=1, prune_eps=1e-9, tier_eps=4e-6, floor_log2=-29.01, mid_log2=-18.01, permax=6,
             mf2=True):
    """The thresholds the host derives for a matrix-core call (CPU tests; on the GPU they are fetched)."""
    _, nks, nmt, _ = geometry(dim)
    c = -0.5 * (2 * np.pi / np.asarray(lbda_nm, dtype=np.float64)) ** 2
    prune = prune_eps > 0
    thr_blk = F32(np.log2(0.5 * prune_eps / (2.0 * ndb * 512 * nmt * nks))) if prune else F32(0)
    tiers = prune and tier_eps > 0
    per, ngr = groups(c.size, permax)
    return Par(thr_blk, F32(floor_log2) if tiers else F32(-1e30), F32(mid_log2) if tiers else F32(-1e30),
               F32(0.5 * tier_eps) if np.isfinite(tier_eps) else F32(0), thr_blk,
               F32(0.5 * prune_eps / (2.0 * dim * ndb)) if prune else F32(0),
               min(F32(x * 1.44269504088896340736) for x in c), per, ngr, c)


# ---- minima ------------------------------------------------------------------------------------------------------

def round_down_to_float(v):
    """The largest float32 not above v (the f64 mode rounds its minima down)."""
    v = np.asarray(v, dtype=np.float64)
    f = v.astype(F32)
    up = f.astype(np.float64) > v
    f[up] = np.nextafter(f[up], F32(-np.inf))
    return f.astype(np.float64)


def plane_minima(d0, f64=False):
    """k_dmin from a stored plane [...][H1][dim]: (dline [...][H1], dblk [...][nmt][nks]) of max(D, 0); a block of the
    last m-tile holds its own lines only."""
    d0 = np.asarray(d0, dtype=np.float64)
    h1, dim = d0.shape[-2:]
    _, nks, nmt, _ = geometry(dim)
    v = np.maximum(d0, 0.0)
    if f64:
        v = round_down_to_float(v)
    per_line = v.reshape(d0.shape[:-1] + (nks, KBL)).min(axis=-1)              # [...][H1][nks]
    return per_line.min(axis=-1), block_minima_of_lines(per_line)


def block_minima_of_lines(dlin, overrun=False):
    """[...][H1][nks] minima per line and block of 32 columns -> [...][nmt][nks]: the minimum over a block's lines, the
    last m-tile over the H1 - 16 (nmt - 1) lines it has.  overrun (a mutation): the last m-tile takes 16 lines, which
    are the first lines of the next task in the buffer."""
    dlin = np.asarray(dlin, dtype=np.float64)
    h1, nks = dlin.shape[-2:]
    nmt = (h1 + MTL - 1) // MTL
    lead = dlin.shape[:-2]
    pad = np.full(lead + (nmt * MTL - h1, nks), np.inf)
    if overrun:
        flat = dlin.reshape(-1, h1, nks)
        nxt = np.roll(flat, -1, axis=0)[:, :nmt * MTL - h1]
        pad = nxt.reshape(lead + nxt.shape[1:])
    full = np.concatenate([dlin, pad], axis=-2)
    return full.reshape(lead + (nmt, MTL, nks)).min(axis=-2)


# ---- (R) k_mf_prep -----------------------------------------------------------------------------------------------

def block_bound(c2, dmin, tlb):
    """e = c2 dmin + tlb, product and sum in float64, rounded once to float32 (the kernel's fma)."""
    with np.errstate(over='ignore', invalid='ignore'):
        e = (np.float64(c2) * np.asarray(dmin, dtype=np.float64) + np.asarray(tlb, dtype=np.float64)).astype(F32)
    return np.where(np.isnan(e), F32(-np.inf), e)


def peak_bound(d0_lines, tel_lines, c2):
    """S: the OTF summed over the first lines of the half plane (line 0 once, the others twice), [ndir][pl][dim] and
    [pl][dim] -> float."""
    d = np.maximum(np.asarray(d0_lines, dtype=np.float64), 0.0)
    if d.ndim == 2:
        d = d[None]
    w = np.full(d.shape[1], 2.0)
    w[0] = 1.0
    return float((w[None, :, None] * np.asarray(tel_lines, dtype=np.float64)[None] * np.exp2(np.float64(c2) * d)).sum())


def tiers(e, par, S, mutate=''):
    """The two thresholds of one (task, wavelength) under the budget tier_half S, from its block bounds e [nmt][nks].
    -> (thr_keep, thr_mid, info); info: what happened ('steps_keep', 'clamp', 'steps_mid', 'no_mid', 'no_tier_block',
    'budget' whether the budget pass ran), 'ratios' mass / budget at every comparison made, 'visited' every threshold a
    block was compared with."""
    thr = par.thr_eps
    thr_keep, thr_mid = max(thr, par.thr_floor), par.thr_mid
    info = dict(steps_keep=0, clamp=False, steps_mid=0, no_mid=False, no_tier_block=False, budget=False, ratios=[],
                visited=[thr])
    ev = e[np.isfinite(e)].astype(np.float64)

    def mass(lo, hi):
        info['visited'] += [lo, hi]
        return 1024.0 * np.exp2(ev[(ev > lo) & (ev <= hi)]).sum()

    if par.tier_half > 0 and max(thr_mid, thr_keep) > thr:
        mf, mm = mass(thr, thr_keep), mass(thr_keep, max(thr_mid, thr_keep))
        if mf > 0 or mm > 0:
            info['budget'] = True
            budget = float(par.tier_half) * S
            info['ratios'].append(mf / budget)
            if mf > budget:
                while True:
                    thr_keep = F32(thr_keep - F32(2))
                    info['steps_keep'] += 1
                    if thr_keep <= thr and mutate != 'no clamp':
                        thr_keep = thr
                        info['clamp'] = True
                        break
                    m = mass(thr, thr_keep)
                    info['ratios'].append(m / budget)
                    if not m > budget:
                        break
                mm = mass(thr_keep, thr_mid)
            lost = 1.0 / (1024.0 if mutate == 'mid 2^-10' else 2048.0)
            while True:
                if not thr_mid > thr_keep:
                    break
                info['ratios'].append(mm * lost / budget)
                if not mm * lost > budget:
                    break
                thr_mid = F32(thr_mid - F32(2))
                info['steps_mid'] += 1
                mm = mass(thr_keep, thr_mid)
        else:
            info['no_tier_block'] = True
    if mutate == 'keep+2':
        thr_keep = F32(thr_keep + F32(2))
    if mutate == 'keep-2':
        thr_keep = F32(thr_keep - F32(2))
    info['visited'] += [thr_keep, thr_mid]
    info['no_mid'] = bool(thr_mid <= thr_keep)
    return thr_keep, thr_mid, info


def bits(mask):
    """[..., nks] bool -> [...] uint64 words, bit ks."""
    mask = np.asarray(mask, dtype=bool)
    w = (np.uint64(1) << np.arange(mask.shape[-1], dtype=np.uint64))
    return (mask * w).sum(axis=-1, dtype=np.uint64)


def unbits(words, nks):
    words = np.asarray(words).astype(np.uint64)
    return ((words[..., None] >> np.arange(nks, dtype=np.uint64)) & np.uint64(1)).astype(bool)


def derive(own, per, ngr, mutate=''):
    """own [tc][nl][nmt][2][nks] bool -> the words and items that follow from it: uni [tc][ngr][nmt][nks],
    ksum [tc][nl][nsw][nks], kuni [tc][ngr][nsw][nks] (bool), gsw [tc][ngr] int, items: a sorted list of
    (class, task, grp, sweep, sweeps), sched [64]."""
    tc, nl, nmt, _, nks = own.shape
    nsw = (nmt + KT2 - 1) // KT2
    any_ = own.any(axis=3)                                             # [tc][nl][nmt][nks]
    uni = np.zeros((tc, ngr, nmt, nks), dtype=bool)
    for g in range(ngr):
        ls = list(range(g * per, min(nl, (g + 1) * per)))
        if mutate.startswith('uni misses wavelength '):
            ls = [l for l in ls if l != int(mutate.split()[-1])]
        uni[:, g] = any_[:, ls].any(axis=1)

    def sweeps(a, short=False):                                        # [..., nmt, nks] -> [..., nsw, nks]
        p = np.zeros(a.shape[:-2] + (nsw * KT2, nks), dtype=bool)
        p[..., :nmt, :] = a
        p = p.reshape(a.shape[:-2] + (nsw, KT2, nks))
        return (p[..., 1:, :] if short else p).any(axis=-2)      # short: without a sweep's first m-tile
    ksum = sweeps(any_, mutate == 'ksum over 7 m-tiles')
    kuni = sweeps(uni)
    gsw = (kuni.any(axis=-1) * (1 << np.arange(nsw))).sum(axis=-1).astype(np.int64)
    pc = np.zeros((tc, ngr, nsw), dtype=np.int64)
    cnt = uni.sum(axis=-1)
    for sw in range(nsw):
        pc[:, :, sw] = cnt[:, :, sw * KT2:(sw + 1) * KT2].sum(axis=-1)
    items = []
    for t in range(tc):
        for g in range(ngr):
            n = bin(int(gsw[t, g])).count('1')
            for sw in range(nsw):
                if kuni[t, g, sw].any():
                    items.append((min(NLISTS - 1, int(pc[t, g, sw]) * (NLISTS // KT2) // nks), t, g, sw, n))
    items.sort()
    sched = np.bincount([i[0] for i in items], minlength=NLISTS)
    return dict(uni=uni, ksum=ksum, kuni=kuni, gsw=gsw, items=items, sched=sched)


def plan(par, dmin, tlb, d0_lines, tel_lines, nopr=False, mutate=''):
    """(R) of k_mf_prep.  dmin [tc][nmt][nks] block minima (from `dminb`, or block_minima_of_lines(`dlin`)), tlb
    [nmt][nks], d0_lines [tc][pl][dim] and tel_lines [pl][dim] the first peak_lines of `dphi0` and `tel`.  nopr:
    prune_eps = 0.  -> dict: own [tc][nl][nmt][2][nks] bool (word 0 full, word 1 mid), e, thr_keep / thr_mid [tc][nl],
    info [tc][nl], and what `derive` gives."""
    dmin = np.asarray(dmin, dtype=np.float64)
    tc, nmt, nks = dmin.shape
    nl = par.c.size
    own = np.zeros((tc, nl, nmt, 2, nks), dtype=bool)
    e = np.zeros((tc, nl, nmt, nks), dtype=F32)
    tk, tm = np.zeros((tc, nl), dtype=F32), np.zeros((tc, nl), dtype=F32)
    info = [[None] * nl for _ in range(tc)]
    if mutate == 'S one line fewer':
        d0_lines, tel_lines = d0_lines[:, :-1], tel_lines[:-1]
    for t in range(tc):
        for l in range(nl):
            c2 = c2_of(par.c[l])
            if nopr:
                own[t, l, :, 0] = True
                info[t][l] = dict(ratios=[], visited=[], budget=False)
                continue
            e[t, l] = block_bound(c2, dmin[t], tlb)
            S = peak_bound(d0_lines[t], tel_lines, c2)
            tk[t, l], tm[t, l], info[t][l] = tiers(e[t, l], par, S, mutate)
            keep = e[t, l] > tk[t, l]
            full = keep & (e[t, l] > tm[t, l])
            own[t, l, :, 0], own[t, l, :, 1] = full, keep & ~full
    out = dict(own=own, e=e, thr_keep=tk, thr_mid=tm, info=info, par=par, nopr=nopr)
    out.update(derive(own, par.per, par.ngr, mutate))
    return out


def fetched_plan(own, uni, ksum, kuni, gsw, sched, items, nks):
    """The debug fetches of one call -> the same shape of dict as `plan` gives (masks as bool arrays)."""
    it = sorted(tuple(int(x) for x in r) for r in np.asarray(items).reshape(-1, 5))
    return dict(own=unbits(own, nks), uni=unbits(uni, nks), ksum=unbits(ksum, nks), kuni=unbits(kuni, nks),
                gsw=np.asarray(gsw).astype(np.int64), sched=np.asarray(sched).astype(np.int64), items=it)


def exemptions(ref, near=1e-4):
    """What the comparison leaves out, from the reference alone: blocks [tc][nl][nmt][nks] whose bound lies within one
    float32 ulp of a threshold they were compared with, and (task, wavelength)s [tc][nl] whose mass / budget came
    within `near` of 1 at a step taken or stopped at."""
    e = ref['e']
    blocks = np.zeros(e.shape, dtype=bool)
    pairs = np.zeros(e.shape[:2], dtype=bool)
    if ref['nopr']:
        return blocks, pairs
    for t in range(e.shape[0]):
        for l in range(e.shape[1]):
            inf = ref['info'][t][l]
            ulp = np.spacing(np.abs(e[t, l]))
            for th in set(float(x) for x in inf['visited']):
                with np.errstate(invalid='ignore'):
                    blocks[t, l] |= np.abs(e[t, l].astype(np.float64) - th) <= ulp
            pairs[t, l] = any(abs(r - 1.0) <= near for r in inf['ratios'])
    return blocks, pairs


def compare_plan(ref, got, near=1e-4):
    """Where a plan differs from (R).  -> (findings, stats).  A finding names its place:
      ('own', task, wavelength, m-tile, k-step, word)      ('uni', task, group, m-tile, k-step)
      ('ksum', task, wavelength, sweep, k-step)            ('kuni', task, group, sweep, k-step)
      ('gsw', task, group, sweep)   ('sched', class)       ('item missing' | 'item extra', (class, task, group, sweep, sweeps))
    The derived words are held to what follows from (R)'s masks with the left-out blocks taken from `got`.  stats:
    blocks compared / left out, (task, wavelength)s and how many of them were left out."""
    blocks, pairs = exemptions(ref, near)
    skip = blocks | pairs[:, :, None, None]
    own = np.where(skip[:, :, :, None, :], got['own'], ref['own'])
    out = [('own',) + tuple(int(i) for i in (t, l, mt, ks, w))
           for t, l, mt, w, ks in zip(*np.nonzero(own != got['own']))]
    want = derive(own, ref['par'].per, ref['par'].ngr)
    for name in ('uni', 'ksum', 'kuni'):
        out += [(name,) + tuple(int(i) for i in ix) for ix in zip(*np.nonzero(want[name] != got[name]))]
    nsw = want['kuni'].shape[2]
    diff = np.bitwise_xor(want['gsw'], got['gsw'])
    out += [('gsw', int(t), int(g), sw) for t, g in zip(*np.nonzero(diff)) for sw in range(nsw) if diff[t, g] >> sw & 1]
    out += [('sched', int(k)) for k in np.nonzero(want['sched'] != got['sched'][:NLISTS])[0]]
    a, b = collections.Counter(want['items']), collections.Counter(got['items'])
    out += [('item missing', i) for i in sorted((a - b).elements())]
    out += [('item extra', i) for i in sorted((b - a).elements())]
    stats = dict(blocks=int(skip.size), blocks_out=int(skip.sum()), pairs=int(pairs.size), pairs_out=int(pairs.sum()))
    return out, stats


def coverage(ref):
    """The classes of the issue's list that occurred in a reference plan, as a set of names."""
    seen = set()
    if ref['nopr']:
        return seen
    for row in ref['info']:
        for i in row:
            if i['no_tier_block']:
                seen.add('no tier block')
            if not i['budget']:
                continue
            if i['steps_keep'] == 0 and i['steps_mid'] == 0:
                seen.add('no lowering')
            if i['steps_keep'] > 0 and not i['clamp']:
                seen.add('keep lowered')
            if i['clamp']:
                seen.add('clamp')
            if i['steps_mid'] > 0 and not i['no_mid']:
                seen.add('mid lowered')
            if i['no_mid']:
                seen.add('no mid block')
    nsw = ref['kuni'].shape[2]
    for g in ref['gsw'].ravel():
        n = bin(int(g)).count('1')
        if n == 1:
            seen.add('one sweep')
        if n > 1:
            seen.add('several sweeps')
        if n < nsw:
            seen.add('sweep without work')
    return seen


# ---- (R) k_vkeep, k_task_order, k_peak_floor ---------------------------------------------------------------------

def line_bounds(tel):
    """B_v = float32 log2 of the largest telescope OTF element of line v."""
    with np.errstate(divide='ignore'):
        return np.log2(np.asarray(tel, dtype=np.float64).max(axis=-1)).astype(F32)


def vkeep(par, dline, tel, near=1e-4, mutate=''):
    """(R) of k_vkeep.  dline [tc][ndir][H1] (k_dmin), tel [H1][dim].  -> (vkeep [tc][npair] int, left_out [tc][npair]:
    the sum came within `near` of thr_sum at the boundary line).  Lines from the top down: vkeep = v + 1 at the first
    line where the sum of 2^(c2 A_v + B_v) exceeds thr_sum (c2 of the pair's longer wavelength), then the running maximum
    over the pairs."""
    A = np.asarray(dline, dtype=np.float64).min(axis=1)                    # [tc][H1]
    B = line_bounds(tel).astype(np.float64)
    nl = par.c.size
    npair = (nl + 1) // 2
    tc, h1 = A.shape
    vk = np.zeros((tc, npair), dtype=np.int64)
    out = np.zeros((tc, npair), dtype=bool)
    thr = float(par.thr_sum)
    pick = min if mutate == 'shorter wavelength' else max
    for p in range(npair):
        c2 = np.float64(F32(F32(pick(par.c[2 * p], par.c[min(2 * p + 1, nl - 1)])) * LOG2E))
        for t in range(tc):
            with np.errstate(over='ignore', invalid='ignore'):
                x = np.exp2(np.nan_to_num(c2 * A[t] + B, nan=-np.inf, neginf=-np.inf))
            s = np.cumsum(x[::-1])[::-1]                                   # s[v] = the lines v and above
            over = np.nonzero(s > thr)[0]
            vk[t, p] = over[-1] + 1 if over.size else 0
            at = [s[over[-1]]] if over.size else []
            if over.size and over[-1] + 1 < h1:
                at.append(s[over[-1] + 1])
            out[t, p] = any(abs(a / thr - 1.0) <= near for a in at)
    if mutate != 'no running maximum':
        vk = np.maximum.accumulate(vk, axis=1)
        # (a pair that takes an earlier pair's count takes its condition too)
        for p in range(1, npair):
            out[:, p] |= out[:, p - 1] & (vk[:, p] == vk[:, p - 1])
    return vk, out


def compare_vkeep(want, left_out, got):
    """-> [(task, pair)] where a fetched vkeep differs from (R) outside the left-out pairs."""
    bad = (np.asarray(got).astype(np.int64) != want) & ~left_out
    return [(int(t), int(p)) for t, p in zip(*np.nonzero(bad))]


def task_order(vk):
    """The tasks by descending vkeep of the last pair, ties by index."""
    key = np.asarray(vk)[:, -1]
    return np.array(sorted(range(key.size), key=lambda t: (-key[t], t)))


def peak_floor(par, d0_lines, tel_lines, dim):
    """(R) of k_peak_floor: thrf [tc] = min(floor, log2(tier_half S_min / (1024 ndir nblocks))), S_min the OTF of the
    shortest wavelength over the first lines and all directions.  d0_lines [tc][ndir][pl][dim]."""
    _, nks, nmt, _ = geometry(dim)
    d0_lines = np.asarray(d0_lines)
    ndir = d0_lines.shape[1]
    S = np.array([peak_bound(d, tel_lines, par.c2min) for d in d0_lines])
    return np.minimum(float(par.thr_floor), np.log2(float(par.tier_half) * S / (1024.0 * ndir * nmt * nks)))


# ---- (G) the guarantee -------------------------------------------------------------------------------------------

def true_otf(d0, tel, c):
    """tel exp(c max(D, 0)) summed over the directions, weighted for both half planes (the lines 0 and dim/2 once, the
    others twice): d0 [ndir][H1][dim] -> [H1][dim].  Its sum is the true peak."""
    d = np.maximum(np.asarray(d0, dtype=np.float64), 0.0)
    if d.ndim == 2:
        d = d[None]
    w = np.full(d.shape[1], 2.0)
    w[0] = w[-1] = 1.0
    return w[:, None] * np.asarray(tel, dtype=np.float64) * np.exp(np.float64(c) * d).sum(axis=0)


def block_sums(a):
    """[H1][dim] -> [nmt][nks] sums over the blocks."""
    h1, dim = a.shape
    _, nks, nmt, _ = geometry(dim)
    p = np.zeros((nmt * MTL, dim))
    p[:h1] = a
    return p.reshape(nmt, MTL, nks, KBL).sum(axis=(1, 3))


def guarantee_blocks(own, e, par, d0, tel, prune_eps, tier_eps, nopr=False):
    """(G) for the masks of k_mf_prep: own [tc][nl][nmt][2][nks] bool (the plan under test), e the block bounds of (R)
    (they only sort the dropped blocks into those under the eps threshold and those the floor tier dropped), d0
    [tc][H1][dim], tel [H1][dim].  -> list of violations (empty: holds), each (what, task, wavelength, mass, bound)."""
    bad = []
    outside = block_sums(np.asarray(tel, dtype=np.float64)) == 0.0
    for t in range(own.shape[0]):
        for l in range(own.shape[1]):
            otf = true_otf(d0[t], tel, par.c[l])
            m = block_sums(otf)
            peak, otf00 = otf.sum(), otf[0, 0]
            full, mid = own[t, l, :, 0], own[t, l, :, 1]
            dropped = ~(full | mid)
            if nopr:
                if dropped.any():
                    bad.append(('dropped without pruning', t, l, float(dropped.sum()), 0.0))
                continue
            if ((full | mid) & outside).any():
                bad.append(('kept outside the support', t, l, float(((full | mid) & outside).sum()), 0.0))
            under = dropped & (e[t, l] <= par.thr_eps)
            checks = [('eps', m[under].sum(), 0.5 * prune_eps * otf00)]
            if np.isfinite(tier_eps):
                checks += [('floor', m[dropped & ~under].sum(), 0.5 * tier_eps * peak),
                           ('mid', m[mid].sum() / 2048.0, 0.5 * tier_eps * peak)]
            bad += [(w, t, l, float(a), float(b)) for w, a, b in checks if not a <= b]
    return bad


def guarantee_lines(vk, par, d0, tel, share):
    """(G) for k_vkeep: the true mass of the lines v >= vkeep of every wavelength of a pair is within `share` (the part of
    prune_eps the lines get) of OTF[0][0] per direction.  d0 [tc][ndir][H1][dim]."""
    bad = []
    nl = par.c.size
    for t in range(vk.shape[0]):
        for l in range(nl):
            otf = true_otf(d0[t], tel, par.c[l])
            mass, bound = otf[int(vk[t, l // 2]):].sum(), share * otf[0, 0]
            if not mass <= bound:
                bad.append(('lines', t, l, float(mass), float(bound)))
    return bad


def guarantee_floor(thrf, par, dminb, tlb, d0, tel, tier_eps):
    """(G) for k_peak_floor: the blocks max(thr_blk, thrf[t]) drops and the eps rule would keep weigh at most
    tier_eps / 2 of the true peak, for every wavelength.  dminb [tc][nmt][nks], d0 [tc][ndir][H1][dim]."""
    bad = []
    for t in range(len(thrf)):
        thr_t = max(float(par.thr_blk), float(F32(thrf[t])))
        for l in range(par.c.size):
            e = block_bound(c2_of(par.c[l]), dminb[t], tlb).astype(np.float64)
            otf = true_otf(d0[t], tel, par.c[l])
            mass, bound = block_sums(otf)[(e <= thr_t) & (e > float(par.thr_blk))].sum(), 0.5 * tier_eps * otf.sum()
            if not mass <= bound:
                bad.append(('task floor', t, l, float(mass), float(bound)))
    return bad
