"""Local-BA Schur back-end (src/local_bundle_adjustment.c:128-250).

CPU: the oracle's chunk loop equals the reference's OWN functions (matrix_add,
invert_block_diagonal_matrix, zero_*, initialize_random_matrix, matmul2 -- compiled from
local_bundle_adjustment.c into oracle/_ref, driven through main's loop by
oracle/ref_lba_harness.c) bit for bit, NaN pattern included (the reference's placeholder
factors make the landmark blocks singular); with real projection factors (as intended) the
pose block equals the dense float64 Schur complement H_PP - H_PL H_LL^-1 H_LP.
GPU (marked): k_lba_schur equals the oracle bit for bit in both modes.
Edge shapes: ragged last chunks (as intended: only the landmarks that exist, NaN in
J's padding never read), every loop form of the kernel, the largest shapes the LDS formula admits
and the refusal past them, a non-zero starting C, a batch; C in guarded buffers."""
import numpy as np
import pytest

from test_factors import scene


def real_window(seed, P=6, L=40, LC=4):
    """every landmark seen by every pose: factor blocks from the oracle's linearisation"""
    ldmk, pose, _, _, _, cam, _ = scene(seed, F=1, L=L, P=P)
    rng = np.random.default_rng(seed + 100)
    lid = np.repeat(np.arange(L), P).astype(np.int32)
    pid = np.tile(np.arange(P), L).astype(np.int32)
    meas = rng.uniform(0, 376, (L * P, 2)).astype(np.float32)
    return ldmk, pose, cam, lid, pid, meas


def chunked(J, P, L, LC, pad=0.0):
    """[L*P, 20] landmark-major factors -> [chunks, P*LC, 20] with entry ci * P + p; the entries
    of landmarks past L in a ragged last chunk hold `pad`"""
    nch = -(-L // LC)
    out = np.full((nch, P * LC, 20), pad, np.float32)
    for l in range(L):
        for p in range(P):
            out[l // LC, (l % LC) * P + p] = J[l * P + p]
    return out


# ------------------------------------------------------------------ edge shapes
RAGGED = [(2, 7, 3), (6, 41, 4), (6, 43, 4)]  # L % LC != 0
LOOP_FORMS = [(2, 6, 3), (3, 12, 1), (2, 28, 14), (8, 8, 4), (19, 5, 1)]
LDS_LIMIT = 64 * 1024


def lds_bytes(P, LC):
    """include/factors.h: 4 (100 + 9 chunk^2 + 6 S chunk + S^2)"""
    S = 6 * P + 1
    return 4 * (100 + 9 * LC * LC + 6 * S * LC + S * S)


P_MAX = max(P for P in range(1, 200) if lds_bytes(P, 1) <= LDS_LIMIT)  # at chunk 1
LC_MAX = max(c for c in range(1, 200) if lds_bytes(2, c) <= LDS_LIMIT)  # at P = 2
LDS_MAX = [(P_MAX, 3, 1), (2, LC_MAX + 2, LC_MAX)]  # the second one ragged: chunks of LC_MAX and 2
LDS_REFUSED = [(P_MAX + 1, 3, 1), (2, LC_MAX + 3, LC_MAX + 1)]
INTENDED_SHAPES = RAGGED + LOOP_FORMS + LDS_MAX
BUILT_SHAPES = [(3, 7, 2)] + LOOP_FORMS + LDS_MAX  # (3, 7, 2): ragged, a whole last chunk as in main

# The oracle's |C - dense float64 Schur complement| / max|H_PP| after the ragged-chunk fix, measured
# over INTENDED_SHAPES with the windows of intended_window() (x86-64, -ffp-contract=off):
#   (2,7,3) 3.32e-6   (6,41,4) 1.50e-6  (6,43,4) 1.24e-6  (2,6,3) 1.53e-5   (3,12,1) 4.48e-6
#   (2,28,14) 2.44e-6 (8,8,4) 5.81e-6   (19,5,1) 4.94e-7  (20,3,1) 1.36e-6  (2,40,38) 3.81e-5
# ((6,40,4) of the test above: 8.15e-7; divisible shapes before the fix: 7.3e-7 .. 4.4e-6).  The
# large ones are P = 2 windows: two observations leave H_LL poorly conditioned, and the same 40
# landmarks in chunks of 2 give 1.8e-4, so it is the window and not the ragged chunk.  Bound: 10 x
# the largest, the margin given to another platform's rounding; never taken from the kernel.
SCHUR_MEASURED_MAX = 3.81e-5
SCHUR_TOL = 10 * SCHUR_MEASURED_MAX


def intended_window(orc, seed, P, L, LC):
    """real factors of real_window, chunked with NaN in a ragged chunk's padding -> (J, Jc)"""
    ldmk, pose, cam, lid, pid, meas = real_window(seed, P, L, LC)
    J = orc.pf_linearize(ldmk, pose, lid, pid, meas, cam)[1]
    return J, chunked(J, P, L, LC, pad=np.nan)


def dense_schur(J, P, L):
    """float64 (H_PP, H_PP - H_PL H_LL^-1 H_LP) of landmark-major factors J [L*P, 20]"""
    Jd = J.reshape(-1, 10, 2).transpose(0, 2, 1).astype(np.float64)  # [F, 2, 10]
    HPP = np.zeros((6 * P, 6 * P))
    Schur = np.zeros((6 * P, 6 * P))
    for l in range(L):
        HLL = np.zeros((3, 3))
        HPL = np.zeros((6 * P, 3))
        for p in range(P):
            Jf = Jd[l * P + p]
            HLL += Jf[:, :3].T @ Jf[:, :3]
            HPL[6 * p:6 * p + 6] += Jf[:, 3:9].T @ Jf[:, :3]
            HPP[6 * p:6 * p + 6, 6 * p:6 * p + 6] += Jf[:, 3:9].T @ Jf[:, 3:9]
        Schur += HPL @ np.linalg.inv(HLL) @ HPL.T
    return HPP, HPP - Schur


def start_C(seed, P):
    """a non-zero starting C of the size of a real window's entries"""
    return (np.random.default_rng(seed).standard_normal((6 * P + 1) ** 2) * 1e4).astype(np.float32)


def test_edge_shapes_are_what_they_claim():
    """every condition the GPU cases rely on (the kernel's loop forms are in k_lba.hip)"""
    for P, L, LC in RAGGED:
        assert L % LC != 0 and P >= 2
    assert all(L % LC != 0 for P, L, LC in BUILT_SHAPES[:1])
    by = {s: s for s in LOOP_FORMS}
    assert by[(3, 12, 1)][2] == 1
    P, L, LC = by[(2, 28, 14)]
    assert 3 * LC == 42 and 3 * LC * 6 * P > 256  # step (4) strides, with a k loop of 42
    P, L, LC = by[(8, 8, 4)]
    assert 36 * P * P == 2304 and 3 * LC * 6 * P > 256  # step (5): 9 trips of 256 threads
    assert lds_bytes(19, 1) == 56096
    assert (P_MAX, LC_MAX) == (20, 38)
    for (P, L, LC), (P2, L2, LC2) in zip(LDS_MAX, LDS_REFUSED):
        assert lds_bytes(P, LC) <= LDS_LIMIT < lds_bytes(P2, LC2)
        assert (P2, LC2) in ((P + 1, LC), (P, LC + 1))
    assert all(P >= 2 for P, L, LC in INTENDED_SHAPES)  # one observation makes H_LL singular
    assert LDS_MAX[1][1] % LDS_MAX[1][2] != 0


@pytest.mark.parametrize("P,L,LC", INTENDED_SHAPES)
def test_oracle_as_intended_edge_shapes_are_the_schur_complement(orc, P, L, LC):
    """ragged shapes included: no NaN although the padding of J is NaN (never read), and the
    dense float64 complement over exactly L landmarks within SCHUR_TOL of max|H_PP|"""
    J, Jc = intended_window(orc, 40 + P + L + LC, P, L, LC)
    assert (L % LC == 0) == (not np.isnan(Jc).any())
    C = orc.lba_schur(P, L, LC, Jc, as_built=False)
    assert not np.isnan(C).any()
    S = 6 * P + 1
    HPP, ref = dense_schur(J, P, L)
    err = np.abs(C.reshape(S, S).T[:6 * P, :6 * P] - ref).max() / np.abs(HPP).max()
    print("schur error (%d, %d, %d): %.2e of max|H_PP|" % (P, L, LC, err))
    assert err <= SCHUR_TOL


def test_oracle_accumulates_in_place(orc):
    """C is accumulated, not overwritten: a non-zero start changes the result, by the start itself
    up to float32 rounding.  Bound: an entry sees L P + 2 chunks 3 LC = 30 float32 additions per
    run at (2, 6, 3), each within 2^-24 of a running value that |start| + max|H_PP| bounds: 60 x
    2^-24 = 3.6e-6 for the two runs together."""
    P, L, LC = 2, 6, 3
    J, Jc = intended_window(orc, 9, P, L, LC)
    C0 = start_C(1, P)
    c, d = orc.lba_schur(P, L, LC, Jc, as_built=False), orc.lba_schur(P, L, LC, Jc, as_built=False, C=C0)
    assert not same_bits(c, d) and not np.isnan(d).any()
    scale = np.abs(C0).max() + np.abs(dense_schur(J, P, L)[0]).max()
    assert np.abs(d.astype(np.float64) - c - C0).max() <= 60 * 2.0 ** -24 * scale


@pytest.mark.parametrize("P,L,LC", [(8, 1000, 4), (3, 20, 2), (5, 36, 3)] + BUILT_SHAPES)
def test_oracle_vs_reference_functions(orc, P, L, LC):
    if not orc.ref_available():
        pytest.skip("reference build absent (GPU box): pinned in the build container")
    C = np.zeros((6 * P + 1) ** 2, np.float32)
    orc.ref_lba().ref_lba_schur_main(P, L, LC, orc._ptr(C))
    C2 = orc.lba_schur(P, L, LC, orc.lba_reference_J(P, L, LC), as_built=True)
    assert (C.view(np.int32) == C2.view(np.int32)).all()


def test_oracle_as_intended_is_the_schur_complement(orc):
    P, L, LC = 6, 40, 4
    ldmk, pose, cam, lid, pid, meas = real_window(7, P, L, LC)
    _, J, _ = orc.pf_linearize(ldmk, pose, lid, pid, meas, cam)
    C = orc.lba_schur(P, L, LC, chunked(J, P, L, LC), as_built=False)
    S = 6 * P + 1
    Cm = C.reshape(S, S).T  # column-major
    HPP, ref = dense_schur(J, P, L)
    assert np.abs(Cm[:6 * P, :6 * P] - ref).max() <= 2e-3 * np.abs(HPP).max()


def same_bits(a, b):
    """bit for bit, except that a NaN is any NaN (x86 makes the negative quiet NaN for 0/0 and
    inf - inf, the GPU the positive one)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return (na == nb).all() and (a[~na].view(np.int32) == b[~nb].view(np.int32)).all()


@pytest.mark.gpu
def test_gpu_lba_schur_bit_exact(ctx, orc, torch_cuda):
    torch = torch_cuda
    dev = torch.device("cuda:0")
    ctx.set_stream(torch.cuda.current_stream())
    # as built: the reference's placeholder factors, two windows in one launch
    P, L, LC = 8, 1000, 4
    Jr = orc.lba_reference_J(P, L, LC)
    C = torch.zeros((2, (6 * P + 1) ** 2), dtype=torch.float32, device=dev)
    ctx.lba_schur(P, L, LC, torch.from_numpy(np.stack([Jr, Jr])).to(dev), C, semantics=0)
    # as intended: real factor blocks, 3 windows
    P2, L2, LC2 = 6, 40, 4
    Js = []
    for s in range(3):
        ldmk, pose, cam, lid, pid, meas = real_window(20 + s, P2, L2, LC2)
        Js.append(chunked(orc.pf_linearize(ldmk, pose, lid, pid, meas, cam)[1], P2, L2, LC2))
    C2 = torch.zeros((3, (6 * P2 + 1) ** 2), dtype=torch.float32, device=dev)
    ctx.lba_schur(P2, L2, LC2, torch.from_numpy(np.stack(Js)).to(dev), C2, semantics=1)
    torch.cuda.synchronize()
    ctx.set_stream(None)
    exp = orc.lba_schur(P, L, LC, Jr, as_built=True)
    for b in range(2):
        assert same_bits(C[b].cpu().numpy(), exp)
    for s in range(3):
        e2 = orc.lba_schur(P2, L2, LC2, Js[s], as_built=False)
        assert same_bits(C2[s].cpu().numpy(), e2) and not np.isnan(e2).any()


def _gpu_schur(ctx, torch, P, L, LC, Js, semantics, C0s=None):
    """one launch over len(Js) windows; C in a guarded buffer, started from C0s (default zero)"""
    from test_gpu_tracks import Guarded

    S = 6 * P + 1
    C = Guarded(torch, (len(Js), S * S), torch.float32)
    start = np.zeros((len(Js), S * S), np.float32) if C0s is None else np.stack(C0s)
    C.t.copy_(torch.from_numpy(start))
    ctx.set_stream(torch.cuda.current_stream())
    try:
        ctx.lba_schur(P, L, LC, torch.from_numpy(np.stack(Js)).to("cuda:0"), C.t, semantics=semantics)
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    return C.np()


@pytest.mark.gpu
@pytest.mark.parametrize("P,L,LC", INTENDED_SHAPES)
def test_gpu_lba_schur_as_intended_edge_shapes(ctx, orc, torch_cuda, P, L, LC):
    """the windows of test_oracle_as_intended_edge_shapes_are_the_schur_complement (NaN in the
    padding of J): the oracle's bits and no NaN"""
    _, Jc = intended_window(orc, 40 + P + L + LC, P, L, LC)
    got = _gpu_schur(ctx, torch_cuda, P, L, LC, [Jc], 1)
    exp = orc.lba_schur(P, L, LC, Jc, as_built=False)
    assert same_bits(got[0], exp) and not np.isnan(got).any()


@pytest.mark.gpu
@pytest.mark.parametrize("P,L,LC", BUILT_SHAPES)
def test_gpu_lba_schur_as_built_edge_shapes(ctx, orc, torch_cuda, P, L, LC):
    """the reference's placeholder factors (pinned to its own functions at these shapes above)"""
    Jr = orc.lba_reference_J(P, L, LC)
    got = _gpu_schur(ctx, torch_cuda, P, L, LC, [Jr], 0)
    assert same_bits(got[0], orc.lba_schur(P, L, LC, Jr, as_built=True))


@pytest.mark.gpu
@pytest.mark.parametrize("P,L,LC", LDS_REFUSED)
def test_gpu_lba_schur_refuses_past_the_lds_limit(ctx, torch_cuda, P, L, LC):
    import mvtrack
    from test_gpu_tracks import FILL, Guarded

    torch = torch_cuda
    S = 6 * P + 1
    C = Guarded(torch, (1, S * S), torch.float32)
    J = torch.zeros((1, -(-L // LC), P * LC, 20), dtype=torch.float32, device="cuda:0")
    for semantics in (0, 1):
        with pytest.raises(mvtrack.MVError):
            ctx.lba_schur(P, L, LC, J, C.t, semantics=semantics)
        assert mvtrack.lib().mv_last_status() == mvtrack.MV_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert (C.np() == FILL).all()


@pytest.mark.gpu
def test_gpu_lba_schur_batch_accumulates_in_place(ctx, orc, torch_cuda):
    """3 windows with different J and different non-zero starting C in one launch, ragged as
    intended and as built: each equals the oracle from the same start, and differs from the zero start"""
    for (P, L, LC), semantics in (((6, 43, 4), 1), ((3, 7, 2), 0)):
        if semantics:
            Js = [intended_window(orc, 60 + s, P, L, LC)[1] for s in range(3)]
        else:
            rng = np.random.default_rng(61)
            Js = [rng.uniform(-2, 2, (-(-L // LC), P * LC, 20)).astype(np.float32) for _ in range(3)]
        C0s = [start_C(70 + s, P) for s in range(3)]
        got = _gpu_schur(ctx, torch_cuda, P, L, LC, Js, semantics, C0s)
        for s in range(3):
            exp = orc.lba_schur(P, L, LC, Js[s], as_built=not semantics, C=C0s[s])
            assert same_bits(got[s], exp), (semantics, s)
            assert not (semantics and np.isnan(exp).any())  # (as built, entry p * ci leaves A singular)
            assert not same_bits(exp, orc.lba_schur(P, L, LC, Js[s], as_built=not semantics)), (semantics, s)
            assert not same_bits(exp, orc.lba_schur(P, L, LC, Js[(s + 1) % 3], as_built=not semantics, C=C0s[s]))
