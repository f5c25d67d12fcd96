"""Deterministic cases and expected values for x265amd_intra_costs (tests/test_intra_costs.py).

The expected values never come from the code under test: the CPU oracle (pyoracle.CpuPrims) supplies
intra_filter, intra_pred, intra_allangs, TRANSPOSE and SA8D, chained in the reference's order
(search.cpp:1250-1343 + 1381-1388, 1488-1558); plain numpy restates the four things the oracle lacks:
strong smoothing (predict.cpp:619-645), scale2D_64to32 / scale1D_128to64 (pixel.cpp:504-547) and the
cost / argmin stage.
"""
from __future__ import annotations

import functools

import numpy as np

from cases import SA8D, TRANSPOSE, Det, pixel_dtype, seed_of

N_JOBS = 37                      # no multiple of any jobs-per-wave count (2, 8, 32)
BEST_DTYPE = np.dtype([("cost", np.uint64), ("sad", np.uint32), ("bits", np.uint32), ("mode", np.uint32),
                       ("reserved", np.uint32)])
assert BEST_DTYPE.itemsize == 24
LAMBDAS = (1, 1500, 1 << 24)     # 1, a mid value, and one at which a single bit outweighs any distortion

# content classes by job index (the 32x32 batch adds the strong-smoothing threshold classes)
FLAT, VERT, HORZ, CLIP = 0, 1, 2, 3
STRONG_BOTH, STRONG_TOP_ONLY, STRONG_LEFT_ONLY, STRONG_AT_M1, STRONG_AT = 4, 5, 6, 7, 8


def _neighbours_and_block(det, cls, log2, depth):
    """one job's source block (S x S) and unfiltered neighbours (4S + 1), S = 1 << log2"""
    S = 1 << log2
    pmax = (1 << depth) - 1
    sc = 1 << (depth - 8)
    fenc = det.ints(0, pmax + 1, S * S).reshape(S, S)
    nb = det.ints(0, pmax + 1, 4 * S + 1)
    above, left = nb[1:2 * S + 1], nb[2 * S + 1:]          # views
    if cls == FLAT:
        fenc[:] = 128 * sc
        nb[:] = 128 * sc
    elif cls == VERT:
        # every row repeats the above neighbours; the left column wobbles around the top-left so the
        # mode-26 edge filter changes the first column
        nb[0] = 100 * sc
        left[:] = 100 * sc + 2 * (np.arange(2 * S) % 3)
        fenc[:] = above[None, :S]
    elif cls == HORZ:
        nb[0] = 100 * sc
        above[:] = 100 * sc + 2 * (np.arange(2 * S) % 3)
        fenc[:] = left[:S, None]
    elif cls == CLIP:
        # 0 / maxval beside a mid-grey top-left: the mode-10/26 edge filter clips at both ends
        nb[0] = 128 * sc
        above[:] = np.where(np.arange(2 * S) % 2 == 0, pmax, 0)
        left[:] = np.where(np.arange(2 * S) % 2 == 0, 0, pmax)
        if log2 == 6:                                      # keep the extremes through the 2:1 scaling
            above[:] = np.where((np.arange(2 * S) // 2) % 2 == 0, pmax, 0)
            left[:] = np.where((np.arange(2 * S) // 2) % 2 == 0, 0, pmax)
    elif log2 == 5 and STRONG_BOTH <= cls <= STRONG_AT:
        # abs(topLeft + last - 2 * middle) against threshold = 1 << (depth - 5), on top and left
        thr = 1 << (depth - 5)
        tl, mid = 100 * sc, 120 * sc
        passing, failing = 2 * mid - tl, 2 * mid - tl + 40 * sc
        nb[0] = tl
        nb[1:] = mid + det.ints(-6 * sc, 6 * sc + 1, 4 * S)   # noisy, so the two smoothings differ
        above[31] = left[31] = mid                         # refBuf[32], refBuf[64 + 32]
        top_last, left_last = {
            STRONG_BOTH: (passing, passing), STRONG_TOP_ONLY: (passing, failing),
            STRONG_LEFT_ONLY: (failing, passing), STRONG_AT_M1: (passing + thr - 1, passing - (thr - 1)),
            STRONG_AT: (passing + thr, passing)}[cls]
        above[2 * S - 1], left[2 * S - 1] = top_last, left_last
    return fenc, nb


@functools.lru_cache(maxsize=None)
def make_batch(log2: int, depth: int, n: int = N_JOBS):
    """inputs of one batch: source blocks at scattered, non-monotonic offsets of a plane (stride 64, or 96 for
    the 64x64 form), neighbours packed at the odd pitch 4S + 1 in another shuffled order, bits and lambda"""
    det = Det(seed_of("intra_costs", log2, depth, n))
    pdt = pixel_dtype(depth)
    S = 1 << log2
    stride = 64 if S <= 32 else 96
    per_row = stride // S if S <= 32 else 1
    bands = (n + per_row - 1) // per_row
    plane = det.ints(0, 1 << depth, bands * S * stride).astype(pdt)
    slots = np.argsort(det.ints(0, 1 << 30, bands * per_row), kind="stable")[:n]
    xs = (slots % per_row) * S if S <= 32 else (slots % 3) * 16
    fenc_off = ((slots // per_row) * S * stride + xs).astype(np.int64)
    pitch = 4 * S + 1
    nb = np.zeros(n * pitch, pdt)
    nb_off = (np.argsort(det.ints(0, 1 << 30, n), kind="stable") * pitch).astype(np.int64)
    p2 = plane.reshape(-1, stride)
    for j in range(n):
        f, b = _neighbours_and_block(det, j, log2, depth)
        y, x = divmod(int(fenc_off[j]), stride)
        p2[y:y + S, x:x + S] = f
        nb[nb_off[j]:nb_off[j] + pitch] = b
    bits = np.stack([det.ints(1, 4, n), det.ints(3, 6, n), det.ints(3, 6, n), det.ints(6, 9, n)], axis=1)
    bits[FLAT] = 5                                         # equal bits: the flat block's tie goes to DC
    lam = np.array([LAMBDAS[(j // 3) % 3] for j in range(n)], np.uint32)
    return dict(log2=log2, depth=depth, n=n, fenc=plane, fenc_stride=stride, fenc_off=fenc_off, nb=nb,
                nb_off=nb_off, bits=np.ascontiguousarray(bits.astype(np.uint32)), lam=lam)


def _scale_64(batch):
    """scale2D_64to32 of every block and scale1D_128to64 of every neighbour array (top-left kept)"""
    n, st = batch["n"], batch["fenc_stride"]
    pdt = batch["fenc"].dtype
    p2 = batch["fenc"].reshape(-1, st).astype(np.int64)
    blocks = np.zeros((n, 32, 32), pdt)
    nbs = np.zeros((n, 129), pdt)
    for j in range(n):
        y, x = divmod(int(batch["fenc_off"][j]), st)
        b = p2[y:y + 64, x:x + 64]
        blocks[j] = (b[0::2, 0::2] + b[0::2, 1::2] + b[1::2, 0::2] + b[1::2, 1::2] + 2) >> 2
        s = batch["nb"][batch["nb_off"][j]:batch["nb_off"][j] + 257].astype(np.int64)
        nbs[j, 0] = s[0]
        nbs[j, 1:] = (s[1::2] + s[2::2] + 1) >> 1
    return blocks, nbs


def _strong_filter(ref, filt, depth):
    """predict.cpp:619-645 on 32x32 jobs: bilinear smoothing where both threshold tests pass"""
    thr = 1 << (depth - 5)
    for j in range(ref.shape[0]):
        s = ref[j].astype(np.int64)
        tl, top_last, left_last = s[0], s[64], s[128]
        if abs(tl + top_last - 2 * s[32]) < thr and abs(tl + left_last - 2 * s[64 + 32]) < thr:
            init = (tl << 6) + 32
            i = np.arange(1, 64)
            f = s.copy()
            f[0] = tl
            f[1:64] = (init + (top_last - tl) * i) >> 6
            f[65:128] = (init + (left_last - tl) * i) >> 6
            f[64], f[128] = top_last, left_last
            filt[j] = f.astype(filt.dtype)


@functools.lru_cache(maxsize=None)
def expected_sad(log2: int, depth: int, strong: int, n: int = N_JOBS) -> np.ndarray:
    """sad[n][35] through the oracle chain, in the reference's order"""
    import torch

    from pyoracle import CpuPrims

    cpu = CpuPrims("oracle", depth)
    batch = make_batch(log2, depth, n)
    pdt = batch["fenc"].dtype
    T = torch.from_numpy
    if log2 == 6:
        N, shift = 32, 2
        blocks, ref = _scale_64(batch)
        fenc, fs = np.ascontiguousarray(blocks.reshape(-1)), 32
        foff = (np.arange(n) * 32 * 32).astype(np.int64)
    else:
        N, shift = 1 << log2, 0
        fenc, fs, foff = batch["fenc"], batch["fenc_stride"], batch["fenc_off"]
        ref = np.stack([batch["nb"][o:o + 4 * N + 1] for o in batch["nb_off"]])
    nbn = 4 * N + 1
    ref = np.ascontiguousarray(ref)
    roff = (np.arange(n) * nbn).astype(np.int64)
    filt = ref.copy()                                      # 4x4 and the 64x64 form: no filtered buffer
    if log2 in (3, 4, 5):
        cpu.intra_filter(depth, N, T(ref.reshape(-1)), T(roff), T(filt.reshape(-1)), T(roff))
        if log2 == 5 and strong:
            _strong_filter(ref, filt, depth)
    bf = np.full(n, 1 if N <= 16 else 0, np.uint8)
    pred = np.zeros(n * N * N, pdt)
    poff = (np.arange(n) * N * N).astype(np.int64)
    out = np.zeros(n, np.int32)
    sad = np.zeros((n, 35), np.int64)

    def sa8d(a, sa, aoff, b, boff):
        cpu.pixelcmp(SA8D, depth, N, N, T(a), sa, T(aoff), T(b), N, T(boff), T(out))
        return out.astype(np.int64) << shift

    # DC from the unfiltered buffer, bFilter = (N <= 16)
    cpu.intra_pred(depth, N, T(pred), N, T(poff), T(ref.reshape(-1)), T(roff), T(np.full(n, 1, np.uint8)), T(bf))
    sad[:, 1] = sa8d(fenc, fs, foff, pred, poff)
    # planar from the filtered buffer for PUs 8..32
    cpu.intra_pred(depth, N, T(pred), N, T(poff), T(filt.reshape(-1)), T(roff), T(np.zeros(n, np.uint8)),
                   T(np.zeros(n, np.uint8)))
    sad[:, 0] = sa8d(fenc, fs, foff, pred, poff)
    # transpose + all angles; modes < 18 compare the transposed source against the untransposed prediction
    fenc_t = np.zeros(n * N * N, pdt)
    cpu.blockop(TRANSPOSE, depth, N, N, T(fenc_t), N, T(poff), T(fenc), fs, T(foff), T(fenc), fs, T(foff))
    angs = np.zeros(n * 33 * N * N, pdt)
    aoff = (np.arange(n) * 33 * N * N).astype(np.int64)
    cpu.intra_allangs(depth, N, T(angs), T(aoff), T(ref.reshape(-1)), T(roff), T(filt.reshape(-1)), T(roff), T(bf))
    for mode in range(2, 35):
        moff = aoff + (mode - 2) * N * N
        sad[:, mode] = sa8d(fenc_t, N, poff, angs, moff) if mode < 18 else sa8d(fenc, fs, foff, angs, moff)
    assert sad.min() >= 0 and sad.max() < (1 << 31)
    sad.setflags(write=False)
    return sad


@functools.lru_cache(maxsize=None)
def mpm_modes(log2: int, depth: int, n: int = N_JOBS) -> np.ndarray:
    """mpm[n][3]: planar and DC among them, angular only, and three modes none of which is the job's
    lowest-distortion mode"""
    sad = expected_sad(log2, depth, 0, n)
    mpm = np.zeros((n, 3), np.uint8)
    for j in range(n):
        if j % 3 == 0:
            mpm[j] = (0, 1, 26)
        elif j % 3 == 1:
            mpm[j] = (10, 26, 18)
        else:
            low = int(np.argmin(sad[j]))
            mpm[j] = [m for m in (2, 3, 4, 5) if m != low][:3]
    mpm.setflags(write=False)
    return mpm


def decide(sad, mpm, bits, lam):
    """cost[n][35] and best[n]: calcRdSADCost per mode, the minimum in the order DC, planar, 2..34, strict <"""
    n = sad.shape[0]
    cost = np.zeros((n, 35), np.uint64)
    best = np.zeros(n, BEST_DTYPE)
    for j in range(n):
        b = [int(bits[j][3])] * 35
        for k in (2, 1, 0):
            b[int(mpm[j][k])] = int(bits[j][k])            # the first match wins
        c = [int(sad[j][m]) + ((b[m] * int(lam[j]) + 128) >> 8) for m in range(35)]
        cost[j] = c
        bm = 1
        for m in [0] + list(range(2, 35)):
            if c[m] < c[bm]:
                bm = m
        best[j] = (c[bm], int(sad[j][bm]), b[bm], bm, 0)
    return cost, best


@functools.lru_cache(maxsize=None)
def expected(log2: int, depth: int, strong: int, n: int = N_JOBS):
    """(sad int32 [n][35], cost uint64 [n][35], best BEST_DTYPE [n]); asserts that the batch exercises what
    it is meant to"""
    batch = make_batch(log2, depth, n)
    sad = expected_sad(log2, depth, strong, n)
    mpm = mpm_modes(log2, depth, n)
    cost, best = decide(sad, mpm, batch["bits"], batch["lam"])
    if n == N_JOBS:
        assert best["mode"][FLAT] == 1 and not sad[FLAT].any(), "flat block: every mode ties, DC first"
        assert int(np.argmin(sad[VERT])) == 26 and int(np.argmin(sad[HORZ])) == 10
        assert any(int(np.argmin(sad[j])) != int(best["mode"][j]) for j in range(n)), "bits never decide"
        if log2 == 5:
            s0, s1 = expected_sad(5, depth, 0, n), expected_sad(5, depth, 1, n)
            differ = {j for j in range(n) if not np.array_equal(s0[j], s1[j])}
            assert {STRONG_BOTH, STRONG_AT_M1} <= differ, "strong smoothing changes nothing"
            assert not differ & {STRONG_TOP_ONLY, STRONG_LEFT_ONLY, STRONG_AT}, "a failed threshold test smoothed"
    for a in (cost, best):
        a.setflags(write=False)
    return sad.astype(np.int32), cost, best
