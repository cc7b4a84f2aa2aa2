"""NumPy fp64 yardstick of the star finder (mpsfr_find_stars, include/mpsfr.h) and the scene the CPU and GPU tests share.

find() restates the contract literally: the five sums of every pixel over its window in row-major tap order (one
vectorised pass over the frame per tap, so every pixel's sums run in that order), the statistic, the peak rule with its
tie-break, the three-point parabola and the sharpness.  It also returns the sums of the absolute terms, out of which
stat_bounds() and row_bounds() derive the a-priori rounding bounds of the parity test:
  every sum of n terms carries at most (n + 2) eps sum|terms| between two correct evaluations (n - 1 additions and up to
  three roundings inside a term, on either side: twice (n + 2) u with the unit roundoff u = eps / 2),
propagated to first order through den, H, b, T, the parabola and the sharpness, plus a few eps for the closing operations.
"""
import numpy as np

NS = 40
EPS = float(np.finfo(np.float64).eps)
FILLER_ORIGIN = -(1 << 30)
TILE = 32                      # the finder's frame tile; only used to place stars on borders
FRAME = (97, 150)
ALPHA, BETA = 3.096, 2.5       # Moffat of the scene: FWHM = 2 alpha sqrt(2^(1/beta) - 1) = 3.5 px


def moffat(cy, cx, shape=(NS, NS)):
    y, x = np.mgrid[:shape[0], :shape[1]]
    return (1.0 + ((y - cy) ** 2 + (x - cx) ** 2) / ALPHA ** 2) ** (-BETA)


_NORM = float(moffat(NS // 2, NS // 2).sum())


def model():
    """The model stamp of the scene: the Moffat centred on pixel (20, 20), sum 1."""
    return moffat(NS // 2, NS // 2) / _NORM


def core(psf, half):
    c = psf.shape[0] // 2
    return np.asarray(psf, dtype=np.float64)[c - half:c + half + 1, c - half:c + half + 1]


def pixels(image, var, dtype=np.float64):
    """(valid, w, D) of the pixel rule: w = 1 / var (1 without var) on valid pixels, else 0; masked data count as 0."""
    d = np.asarray(image, dtype=np.float64)
    ok = np.isfinite(d)
    v = np.ones(d.shape) if var is None else np.asarray(var, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        ok = ok & np.isfinite(v) & (v > 0)
    one = np.ones((), dtype=dtype)
    w = np.where(ok, one / np.where(ok, v, 1.0).astype(dtype), 0 * one)
    return ok, w, np.where(ok, d, 0.0).astype(dtype)


def sums(image, var, K, dtype=np.float64):
    """S (5, ny, nx) and the sums A of the absolute terms, in row-major tap order; nvalid (ny, nx); valid (ny, nx)."""
    ok, w, d = pixels(image, var, dtype)
    ny, nx = ok.shape
    W = K.shape[0]
    h = W // 2
    wp, dp = np.pad(w, h), np.pad(d, h)
    vp = np.pad(ok, h)
    S, A = np.zeros((5, ny, nx), dtype=dtype), np.zeros((5, ny, nx), dtype=dtype)
    nvalid = np.zeros((ny, nx), dtype=np.int64)
    for a in range(W):
        for b in range(W):
            k = K[a, b].astype(dtype)
            ws, ds = wp[a:a + ny, b:b + nx], dp[a:a + ny, b:b + nx]
            terms = (ws, ws * k, ws * k * k, ws * ds, ws * k * ds)
            for i, t in enumerate(terms):
                S[i] += t
                A[i] += np.abs(t)
            nvalid += vp[a:a + ny, b:b + nx]
    return S, A, nvalid, ok


def statistic(S, nvalid, ok, ntap, usevar):
    """(T, H, b, den): T NaN where it is not defined."""
    with np.errstate(all='ignore'):
        den = S[2] - S[1] * S[1] / S[0]
        H = (S[4] - S[1] * S[3] / S[0]) / den
        b = (S[3] - H * S[1]) / S[0]
        T = H * np.sqrt(den) if usevar else H.copy()
        defined = ok & (2 * nvalid > ntap) & (den > 0)
    return np.where(defined, T, np.nan), H, b, den


def peaks(T, sep, threshold):
    """The flat indices of the peaks, increasing."""
    ny, nx = T.shape
    index = np.arange(ny * nx).reshape(ny, nx)
    with np.errstate(invalid='ignore'):
        cand = np.flatnonzero(T.ravel() >= threshold)
    out = []
    for i in cand:
        Y, X = divmod(int(i), nx)
        sl = (slice(max(Y - sep, 0), Y + sep + 1), slice(max(X - sep, 0), X + sep + 1))
        win, j, t = T[sl], index[sl], T[Y, X]
        with np.errstate(invalid='ignore'):
            rival = np.isfinite(win) & ((win > t) | ((win == t) & (j < i)))
        if not rival.any():
            out.append(int(i))
    return np.array(out, dtype=np.int64)


def parabola(tm, t0, tp):
    """(offset, flagged) of the three-point parabola; the offset is 0 where it has no top."""
    curv = tm - 2.0 * t0 + tp
    if not (np.isfinite(tm) and np.isfinite(tp)) or not curv < 0:
        return 0.0, True
    return float(min(max(0.5 * (tm - tp) / curv, -0.5), 0.5)), False


def find(image, var, psf, half=3, sep=3, threshold=5.0, max_stars=None, dtype=np.float64):
    """The finder on a frame.  Returns a dict: rows (n, 8), origin (n, 2) int32, count (all the peaks of the frame; n =
    min(count, max_stars)), map T, index (the n peak pixels), and S, A, nvalid, H, b, den, K for the bounds."""
    image = np.asarray(image, dtype=np.float64)
    K = core(psf, half)
    S, A, nvalid, ok = sums(image, var, K, dtype)
    usevar = var is not None
    T, H, b, den = statistic(S, nvalid, ok, K.size, usevar)
    idx = peaks(T.astype(np.float64), sep, threshold)
    count = len(idx)
    if max_stars is not None:
        idx = idx[:max_stars]
    ny, nx = image.shape
    _, _, d = pixels(image, var, dtype)
    rows = np.empty((len(idx), 8))
    aux = []
    for r, i in enumerate(idx):
        Y, X = divmod(int(i), nx)
        t0 = T[Y, X]
        nan = np.nan
        dy, fy = parabola(T[Y - 1, X] if Y > 0 else nan, t0, T[Y + 1, X] if Y + 1 < ny else nan)
        dx, fx = parabola(T[Y, X - 1] if X > 0 else nan, t0, T[Y, X + 1] if X + 1 < nx else nan)
        flags = int(fy) | int(fx) << 1
        # the other valid pixels of the window, in tap order
        sd, sk, ad, ak, other = 0.0, 0.0, 0.0, 0.0, 0
        for a in range(-half, half + 1):
            for c in range(-half, half + 1):
                y, x = Y + a, X + c
                if (a or c) and 0 <= y < ny and 0 <= x < nx and ok[y, x]:
                    sd, sk = sd + d[y, x], sk + K[a + half, c + half]
                    ad, ak = ad + abs(d[y, x]), ak + abs(K[a + half, c + half])
                    other += 1
        sharp = np.nan
        if other:
            sden = H[Y, X] * (K[half, half] - sk / other)
            if sden != 0:
                sharp = (d[Y, X] - sd / other) / sden
        if np.isnan(sharp):
            flags |= 4
        rows[r] = (Y + dy, X + dx, t0, H[Y, X], b[Y, X], sharp, nvalid[Y, X], flags)
        aux.append((sd, sk, ad, ak, other, d[Y, X]))
    origin = np.array([(int(i) // nx - NS // 2, int(i) % nx - NS // 2) for i in idx], dtype=np.int32).reshape(-1, 2)
    return dict(rows=rows, origin=origin, count=count, map=T, index=idx, S=S, A=A, nvalid=nvalid, H=H, b=b, den=den,
                K=K, usevar=usevar, aux=aux, shape=(ny, nx))


def stat_bounds(ref):
    """(dT, dH, db) per pixel: the first-order rounding bounds of the module docstring."""
    S, A, ntap = ref['S'], ref['A'], ref['K'].size
    g = (ntap + 2) * EPS
    with np.errstate(all='ignore'):
        dS = g * A
        r = S[1] / S[0]
        den, H, b = ref['den'], ref['H'], ref['b']
        dnum = dS[4] + np.abs(S[3] / S[0]) * dS[1] + np.abs(r) * dS[3] + np.abs(r * S[3] / S[0]) * dS[0] \
            + 4 * EPS * (np.abs(S[4]) + np.abs(r * S[3]))
        dden = dS[2] + 2 * np.abs(r) * dS[1] + r * r * dS[0] + 4 * EPS * (np.abs(S[2]) + np.abs(r * S[1]))
        dH = dnum / np.abs(den) + np.abs(H / den) * dden + 2 * EPS * np.abs(H)
        db = (dS[3] + np.abs(H) * dS[1] + np.abs(S[1]) * dH) / S[0] + np.abs(b) / S[0] * dS[0] \
            + 4 * EPS * (np.abs(S[3]) + np.abs(H * S[1])) / S[0]
        if ref['usevar']:
            root = np.sqrt(den)
            dT = root * dH + np.abs(H) * dden / (2 * root) + 2 * EPS * np.abs(H * root)
        else:
            dT = dH
    return dT, dH, db


def row_bounds(ref):
    """(n, 8) bounds of the rows of `ref` (0 for the discrete columns 6 and 7)."""
    dT, dH, db = stat_bounds(ref)
    T, K = ref['map'], ref['K']
    ny, nx = ref['shape']
    half = K.shape[0] // 2
    out = np.zeros((len(ref['index']), 8))

    def axis(tm, t0, tp, em, e0, ep):
        curv = tm - 2 * t0 + tp
        if not (np.isfinite(tm) and np.isfinite(tp)) or not curv < 0:
            return 0.0
        numr = tm - tp
        dnumr = em + ep + 2 * EPS * (abs(tm) + abs(tp))
        dcurv = em + 2 * e0 + ep + 4 * EPS * (abs(tm) + 2 * abs(t0) + abs(tp))
        off = 0.5 * numr / curv
        return 0.5 * (dnumr / abs(curv) + abs(numr) / curv ** 2 * dcurv) + 2 * EPS * abs(off)

    for r, i in enumerate(ref['index']):
        Y, X = divmod(int(i), nx)
        if 0 < Y < ny - 1:
            out[r, 0] = axis(T[Y - 1, X], T[Y, X], T[Y + 1, X], dT[Y - 1, X], dT[Y, X], dT[Y + 1, X])
        if 0 < X < nx - 1:
            out[r, 1] = axis(T[Y, X - 1], T[Y, X], T[Y, X + 1], dT[Y, X - 1], dT[Y, X], dT[Y, X + 1])
        out[r, 0] += 2 * EPS * Y
        out[r, 1] += 2 * EPS * X
        out[r, 2], out[r, 3], out[r, 4] = dT[Y, X], dH[Y, X], db[Y, X]
        sd, sk, ad, ak, other, d0 = ref['aux'][r]
        sharp = ref['rows'][r, 5]
        if other and np.isfinite(sharp):
            H = ref['H'][Y, X]
            k0 = K[half, half]
            md, mk = sd / other, sk / other
            dnumr = (other + 2) * EPS * ad / other + 2 * EPS * (abs(d0) + abs(md))
            dmk = (other + 2) * EPS * ak / other + 2 * EPS * (abs(k0) + abs(mk))
            denr = H * (k0 - mk)
            ddenr = abs(k0 - mk) * dH[Y, X] + abs(H) * dmk + 2 * EPS * abs(denr)
            out[r, 5] = dnumr / abs(denr) + abs(sharp / denr) * ddenr + 2 * EPS * abs(sharp)
    return out


# ---- the shared scene
HOT = (53, 80)                # the single hot pixel
HOT_VALUE = 400.0
BACK = 10.0
THRESHOLD = {True: 5.0, False: 60.0}     # of the parity settings: 5 sigma with var; without, T is the amplitude (sigma_H ~ 12)
_SCENE = {}


def scene():
    """The 97 x 150 scene: background 10, a variance plane in 0.5 .. 1.5 with matching Gaussian noise, 1 % NaN pixels
    (none on the 3 x 3 pixels around a star's centre or on the hot pixel's window centre), Moffat stars of FWHM 3.5 px
    and flux 300 .. 3000 on a 13-px grid jittered by +-2.5 px -- some of them moved so that their peak pixels lie on the
    rows and columns 31, 32, 63, 64 (the tile borders), within 2 px of each of the four edges and of two corners --, one
    star centred 0.8 px off the frame, and one hot pixel.  Returns a dict: image, var, psf, truth (n, 2), flux (n,),
    hot."""
    if _SCENE:
        return _SCENE
    rng = np.random.default_rng(77)
    ny, nx = FRAME
    pos = {}
    for i in range(7):
        for j in range(11):
            pos[i, j] = (8 + 13 * i + rng.uniform(-2.5, 2.5), 8 + 13 * j + rng.uniform(-2.5, 2.5))
    # peak pixels on the tile borders: rows (columns) 31, 32, 63, 64 -- and the four corners where two borders cross
    for (i, j), y in (((2, 1), 31.2), ((2, 3), 31.8), ((2, 6), 32.3), ((4, 1), 62.9), ((4, 7), 63.6), ((4, 9), 64.2)):
        pos[i, j] = (y, pos[i, j][1])
    for (i, j), x in (((0, 2), 31.3), ((3, 2), 32.2), ((1, 4), 62.8), ((3, 4), 63.7), ((6, 4), 64.1), ((5, 2), 30.9)):
        pos[i, j] = (pos[i, j][0], x)
    pos[2, 2], pos[2, 4], pos[4, 2], pos[4, 4] = (31.4, 31.7), (32.2, 62.9), (63.3, 32.4), (64.1, 63.8)
    # the edges and two corners
    pos[0, 3], pos[6, 6], pos[3, 0], pos[2, 10] = (1.3, pos[0, 3][1]), (95.2, pos[6, 6][1]), (pos[3, 0][0], 0.8), \
        (pos[2, 10][0], 148.6)
    pos[0, 0], pos[6, 10] = (1.2, 1.4), (95.5, 148.3)
    truth = [pos[k] for k in sorted(pos)] + [(-0.8, 75.3)]
    truth = np.array(truth)
    flux = rng.uniform(300, 3000, len(truth))
    var = rng.uniform(0.5, 1.5, FRAME)
    image = BACK + rng.normal(size=FRAME) * np.sqrt(var)
    for (cy, cx), f in zip(truth, flux):
        image += f * moffat(cy, cx, FRAME) / _NORM
    image[HOT] += HOT_VALUE
    nan = rng.uniform(size=FRAME) < 0.01
    for cy, cx in list(truth) + [HOT]:
        y, x = int(np.rint(cy)), int(np.rint(cx))
        nan[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = False
    image[nan] = np.nan
    _SCENE.update(image=image, var=var, psf=model(), truth=truth, flux=flux, hot=HOT)
    return _SCENE


_REF = {}


def scene_reference(usevar=True, half=3, sep=3, threshold=5.0):
    """find() on the scene, computed once per setting and left unchanged."""
    key = (usevar, half, sep, threshold)
    if key not in _REF:
        s = scene()
        _REF[key] = find(s['image'], s['var'] if usevar else None, s['psf'], half, sep, threshold)
    return _REF[key]


def embed(a, shape, offset, fill=np.nan):
    """`a` inside a frame of `shape` at `offset`, `fill` around it."""
    out = np.full(shape, fill)
    out[offset[0]:offset[0] + a.shape[0], offset[1]:offset[1] + a.shape[1]] = a
    return out
