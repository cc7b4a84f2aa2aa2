"""The identity behind the Hermitian fold of stage A's column pass, stated in NumPy.

The structure function needs only Re FFT2 of the 80 x 80 patch P.  With T[su][y] the row transforms
of the patch and  Th[su] = (T[su] + conj(T[-su])) / 2,

    Re sum_su T[su] W^(su x) = sum_su Th[su] W^(su x),        Th[-su] = conj(Th[su]),

for ANY real patch -- no point symmetry of the PSD is assumed -- so 41 values Th[0..40] per line are
all the column pass has to read.  The lone edge row su = -40 is its own pair: Th[-40] = T[-40] / 2,
Th[+40] = conj(T[-40]) / 2.  The kernel stores U[su] = c Th[su] with c = 1 for su = 0 and c = 2
otherwise (a pair counts twice; the doubling is exact), folds su = r + Q j into the classes
r = 0 .. Q/2 only (S_(Q-r) = conj(S_r)) and finishes with a Q-point complex-to-real transform.

This test mirrors that arithmetic for the three lane layouts whose edge term falls differently:
N = 128 (L = 16, Q = 8: su = +-40 in class 0), N = 512 (L = 32, Q = 16: class Q/2 = 8) and
N = 1280 (L = 64, Q = 20: class 0).
"""
import numpy as np
import pytest

NAO = 80
H = NAO // 2

# lanes per line of the column pass (series_lanes<N>() in stage_a2.hip)
LANES = {128: 16, 512: 32, 1280: 64}


def _row_pass(P, N):
    """T[su + 40][y] = sum_sv P[su + 40][sv + 40] exp(-2 pi i sv y / N), y = 0 .. N/2."""
    sv = np.arange(-H, H)
    y = np.arange(N // 2 + 1)
    return P @ np.exp(-2j * np.pi * np.outer(sv, y) / N)


def _hermitian_half(T):
    """U[su][y], su = 0 .. 40: the 41 stored values of a line (c Th, see the module docstring)."""
    U = np.empty((H + 1, T.shape[1]), dtype=complex)
    U[0] = T[H].real                                   # su = 0: Th[0] = Re T[0], counted once
    for su in range(1, H):
        U[su] = T[H + su] + np.conj(T[H - su])         # 2 Th[su]
    U[H] = np.conj(T[0])                               # 2 Th[40] = conj(T[-40]): the edge row alone
    return U


def _fold_c2r(U, N, L):
    """Re X[y][x], x = L k1 + k2, from the 41 stored values of every line y: the classes r = 0 .. Q/2
    of su = r + Q j, each lane's factor W_N^(r k2) and a Q-point complex-to-real transform."""
    Q = N // L
    assert H % Q in (0, Q // 2), 'the edge term falls in a self-conjugate class'
    k2 = np.arange(L)
    ny = U.shape[1]
    S = np.zeros((Q // 2 + 1, ny, L), dtype=complex)
    for r in range(Q // 2 + 1):
        for j in range(-(H // Q) - 1, H // Q + 2):
            su = r + Q * j
            if abs(su) > H:
                continue
            if r == 0 and j >= 0:
                continue                # class 0: U[0] below, the pairs through their negative member
            if 2 * r == Q and j < 0:
                continue                # class Q/2: the pairs through their positive member
            u = U[su] if su >= 0 else np.conj(U[-su])
            S[r] += u[:, None] * np.exp(-2j * np.pi * j * k2 / L)[None, :]
        S[r] *= np.exp(-2j * np.pi * r * k2 / N)[None, :]
    # the self-conjugate classes are real: a pair contributes u + conj(u)
    S[0] = S[0].real + U[0].real[:, None]
    if Q > 1:
        S[Q // 2] = S[Q // 2].real
    # U carries the factor 2 of the pairs; S_r + S_(Q-r) W^.. = 2 Re(..) is what irfft forms from the
    # half spectrum, so the general classes go in halved
    S[1:Q // 2] *= 0.5
    # X[k1] = sum_r S_r exp(-2 pi i r k1 / Q) over the Hermitian extension = Q irfft(conj(S))
    X = Q * np.fft.irfft(np.conj(S), n=Q, axis=0)          # [k1][y][k2]
    return X.transpose(1, 0, 2).reshape(ny, N)             # x = L k1 + k2


@pytest.mark.parametrize('N', [128, 512, 1280])
def test_hermitian_fold_equals_real_part_of_fft2(N):
    rng = np.random.default_rng(1000 + N)
    # deliberately NOT point-symmetric, and with a strong edge row su = -40
    P = rng.random((NAO, NAO)) * np.linspace(0.2, 3.0, NAO)[:, None]
    P[0] *= 5.0
    assert np.abs(P - P[::-1, ::-1]).max() > 0.1
    E = np.zeros((N, N))
    idx = np.arange(-H, H) % N
    E[np.ix_(idx, idx)] = P
    ref = np.fft.fft2(E).real[:, :N // 2 + 1].T            # [y][x]
    U = _hermitian_half(_row_pass(P, N))
    assert U.shape[0] == 41
    got = _fold_c2r(U, N, LANES[N])
    err = np.abs(got - ref).max() / P.sum()
    assert err < 1e-13, err


@pytest.mark.parametrize('N', [128, 512, 1280])
def test_edge_row_matters(N):
    """Dropping the su = -40 row from the 41 stored values is visible far above the tolerance: the
    test above does pin its handling."""
    rng = np.random.default_rng(2000 + N)
    P = rng.random((NAO, NAO))
    T = _row_pass(P, N)
    U = _hermitian_half(T)
    full = _fold_c2r(U, N, LANES[N])
    U[H] = 0.0
    cut = _fold_c2r(U, N, LANES[N])
    assert np.abs(full - cut).max() / P.sum() > 1e-4
