"""x265amd_inter_costs: the fused merge / bidir candidate evaluation (motion compensation + SA8D per candidate,
cost, winner and the winner's prediction) against the oracle chain of tests/inter_cost_cases.py — exact
equality on every element."""
import ctypes

import numpy as np
import pytest

import inter_cost_cases as icc

SIZES = (3, 4, 5, 6)
EINVAL = 1000


# ---------------------------------------------------------------- CPU: the ABI surface (no device)
@pytest.fixture(scope="module")
def lib(native_lib):
    lib = ctypes.CDLL(native_lib)
    lib.x265amd_sizeof.argtypes = [ctypes.c_char_p]
    return lib


def test_entry_is_exported(lib):
    assert hasattr(lib, "x265amd_inter_costs")


def test_descriptor_sizes_match(lib):
    from src.x265_amd.native import InterBest, InterCostBatch

    assert lib.x265amd_sizeof(b"x265amd_inter_best") == ctypes.sizeof(InterBest) == icc.BEST_DTYPE.itemsize == 24
    assert lib.x265amd_sizeof(b"x265amd_inter_cost_batch") == ctypes.sizeof(InterCostBatch) > 0


def test_abi_version_unchanged(lib):
    assert lib.x265amd_abi_version() == 2


CHROMA_IN = ("fenc_cb", "fenc_cr", "fenc_coff", "ref_cb", "ref_cr", "ref_coff")
PRED_C = ("pred_cb", "pred_cr", "pred_coff")


def _desc(**kw):
    """a descriptor whose pointers are small non-null integers: validation must reject before any is used"""
    from src.x265_amd.native import InterCostBatch

    d = dict(log2_size=3, n=1, max_cand=5, fenc=8, fenc_stride=64, fenc_off=8, ref=8, ref_stride=64, ref_off=8, dir=8,
             mv=8, bits=8, lambda_=8, fenc_cb=8, fenc_cr=8, fenc_cstride=32, fenc_coff=8, ref_cb=8, ref_cr=8,
             ref_cstride=32, ref_coff=8, sad=8, cost=8, best=8, pred=8, pred_stride=64, pred_off=8, pred_cb=8,
             pred_cr=8, pred_cstride=32, pred_coff=8)
    d.update(kw)
    return (InterCostBatch * 1)(InterCostBatch(**d))


def _none(*names):
    return {k: None for k in names}


INVALID = [
    ("depth", 9, 1, {}),
    ("log2_size below", 8, 1, dict(log2_size=2)),
    ("log2_size above", 8, 1, dict(log2_size=7)),
    ("max_cand below", 8, 1, dict(max_cand=0)),
    ("max_cand above", 8, 1, dict(max_cand=6)),
    ("n < 0", 8, 1, dict(n=-1)),
    ("count < 0", 8, -1, {}),
    ("fenc NULL", 8, 1, dict(fenc=None)),
    ("ref NULL", 8, 1, dict(ref=None)),
    ("dir NULL", 8, 1, dict(dir=None)),
    ("mv NULL", 8, 1, dict(mv=None)),
    ("fenc_off NULL", 8, 1, dict(fenc_off=None)),
    ("ref_off NULL", 8, 1, dict(ref_off=None)),
    ("pred_off NULL", 8, 1, dict(pred_off=None)),
] + [("chroma without " + k, 8, 1, {k: None}) for k in CHROMA_IN] + [
    ("chroma only " + k, 8, 1, {**_none(*CHROMA_IN, *PRED_C), k: 8}) for k in CHROMA_IN] + [
    ("pred chroma without " + k, 8, 1, {k: None}) for k in PRED_C] + [
    ("pred_cb without chroma inputs", 8, 1, _none(*CHROMA_IN)),
    ("cost without bits", 8, 1, dict(bits=None, best=None, **_none("pred", "pred_off", *PRED_C))),
    ("best without lambda", 8, 1, dict(lambda_=None, cost=None, **_none("pred", "pred_off", *PRED_C))),
    ("pred without bits", 8, 1, dict(bits=None, cost=None, best=None)),
    ("pred without lambda", 8, 1, dict(lambda_=None, cost=None, best=None)),
    ("no output", 8, 1, _none("sad", "cost", "best", "pred", "pred_off", *PRED_C)),
]


@pytest.mark.parametrize("what,depth,count,kw", INVALID, ids=[c[0].replace(" ", "_") for c in INVALID])
def test_invalid_calls_rejected_without_launch(lib, what, depth, count, kw):
    assert lib.x265amd_inter_costs(depth, count, _desc(**kw), None) == EINVAL, what


def test_second_batch_invalid_rejects_whole_call(lib):
    from src.x265_amd.native import InterCostBatch

    arr = (InterCostBatch * 2)(InterCostBatch(3, 0), _desc(log2_size=9)[0])
    assert lib.x265amd_inter_costs(8, 2, arr, None) == EINVAL


def test_empty_calls_are_noops(lib):
    from src.x265_amd.native import InterCostBatch

    assert lib.x265amd_inter_costs(8, 0, None, None) == 0
    assert lib.x265amd_inter_costs(10, 1, (InterCostBatch * 1)(InterCostBatch(4, 0, 5)), None) == 0


# ---------------------------------------------------------------- CPU: the expected-value builder checks itself
@pytest.mark.parametrize("depth", [8, 10])
def test_builder_zero_mv_bi_equals_pixelavg(oracle_libs, depth):
    """the coincident-block estimate of checkBidir2Nx2N: addAvg of two p2s planes is (a + b + 1) >> 1"""
    chain, avg = icc.zero_mv_bi_is_pixelavg(4, depth)
    assert np.array_equal(chain, avg)


@pytest.mark.parametrize("depth", [8, 10])
def test_builder_hvpp_equals_hps_then_vsp(oracle_libs, depth):
    table, two_step = icc.uni_2d_luma_two_routes(4, depth)
    assert np.array_equal(table, two_step)


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("log2", SIZES)
def test_builder_content(oracle_libs, depth, log2):
    """the content assertions of make_batch / expected hold at every size, with and without chroma"""
    icc.expected(log2, depth, chroma=False)
    e = icc.expected(log2, depth)
    assert e["best"]["cand"][icc.ALLDEAD] == -1 and (e["sad"][icc.ALLDEAD] == icc.DEAD_SAD).all()


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def prims(native_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a gfx950 device"
    from src.x265_amd import Primitives

    return Primitives(device=0)


SENTINEL = 0x5A
PAD = 64                         # bytes of sentinel on each side of an output
PRED_PAD = 12                    # sentinel pixels around a CU's slot of a prediction plane


class Outputs:
    """sad / cost / best device buffers for n CUs of K slots, each between PAD sentinel bytes, and the three
    prediction planes: sentinel-filled, one slot per CU at shuffled positions, stride wider than the CU"""

    def __init__(self, n, K, N, depth, which=("sad", "cost", "best", "pred", "pred_c")):
        import torch

        self.n, self.K, self.N = n, K, N
        self.pdt = icc.pixel_dtype(depth)
        size = dict(sad=K * 4, cost=K * 8, best=24)
        self.box = {k: torch.full((n * size[k] + 2 * PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
                    for k in which if k in size}
        self.planes = {}
        order = np.argsort((np.arange(n) * 7919) % 13, kind="stable")        # a fixed shuffle of the slots
        for k, S in (("pred", N), ("pred_c", N // 2)):
            if k not in which:
                continue
            stride = S + 2 * PRED_PAD + 1                  # odd, wider than the CU
            rows = n * (S + PRED_PAD) + PRED_PAD
            off = np.array([(PRED_PAD + int(order[j]) * (S + PRED_PAD)) * stride + PRED_PAD for j in range(n)], np.int64)
            names = ("pred",) if k == "pred" else ("pred_cb", "pred_cr")
            fill = np.full(rows * stride, SENTINEL | (SENTINEL << 8), np.uint16).astype(self.pdt)
            self.planes[k] = dict(stride=stride, rows=rows, off=off, fill=fill, S=S, names=names,
                                  off_dev=torch.from_numpy(off).to("cuda"),
                                  dev={nm: torch.from_numpy(fill.copy()).to("cuda") for nm in names})

    def get(self, k):
        return self.box[k][PAD:] if k in self.box else None

    def read(self):
        """(outputs as numpy, sentinel padding intact)"""
        out, ok = {}, True
        for k, box in self.box.items():
            h = box.cpu().numpy()
            ok = ok and (h[:PAD] == SENTINEL).all() and (h[-PAD:] == SENTINEL).all()
            body = h[PAD:-PAD]
            out[k] = (body.view(np.uint32).reshape(self.n, self.K) if k == "sad" else
                      body.view(np.uint64).reshape(self.n, self.K) if k == "cost" else body.view(icc.BEST_DTYPE))
        for p in self.planes.values():
            for nm in p["names"]:
                out[nm] = p["dev"][nm].cpu().numpy()
        return out, bool(ok)

    def want_plane(self, name, blocks, live):
        """the whole expected plane: sentinel everywhere but the live CUs' slots"""
        p = self.planes["pred" if name == "pred" else "pred_c"]
        w = p["fill"].copy().reshape(p["rows"], p["stride"])
        for j in range(self.n):
            if live[j]:
                y, x = divmod(int(p["off"][j]), p["stride"])
                w[y:y + p["S"], x:x + p["S"]] = blocks[j]
        return w.reshape(-1)


class DeviceBatch:
    """one batch's inputs on the device; item() makes the inter_cost_batches dict for a CU range"""

    def __init__(self, log2, depth, K=icc.K_MERGE):
        import torch

        b = icc.make_batch(log2, depth, K)
        self.log2, self.depth, self.K, self.n, self.b = log2, depth, K, b["n"], b
        dev = lambda a: torch.from_numpy(np.array(a)).to("cuda")          # (a copy: the cached cases are shared)
        self.t = {k: dev(b[k]) for k in ("fenc", "fenc_off", "ref", "ref_off", "dir", "mv", "fenc_cb", "fenc_cr",
                                         "fenc_coff", "ref_cb", "ref_cr", "ref_coff")}
        self.t["bits"] = dev(b["bits"].view(np.int32))
        self.t["lam"] = dev(b["lam"].view(np.int32))

    def item(self, outs, chroma=True, rd=True, j0=0, j1=None):
        j1 = self.n if j1 is None else j1
        K, t, b = self.K, self.t, self.b
        it = dict(log2_size=self.log2, max_cand=K, fenc=t["fenc"], fenc_stride=b["fenc_stride"],
                  fenc_off=t["fenc_off"][j0:j1], ref=t["ref"], ref_stride=b["ref_stride"],
                  ref_off=t["ref_off"][j0 * K * 2:], dir=t["dir"][j0 * K:], mv=t["mv"][j0 * K * 4:],
                  sad=outs.get("sad"), cost=outs.get("cost"), best=outs.get("best"))
        if rd:
            it.update(bits=t["bits"][j0 * K:], lam=t["lam"][j0:])
        if chroma:
            it.update(fenc_cb=t["fenc_cb"], fenc_cr=t["fenc_cr"], fenc_cstride=b["fenc_cstride"],
                      fenc_coff=t["fenc_coff"][j0:j1], ref_cb=t["ref_cb"], ref_cr=t["ref_cr"],
                      ref_cstride=b["ref_cstride"], ref_coff=t["ref_coff"][j0 * K * 2:])
        if "pred" in outs.planes:
            p = outs.planes["pred"]
            it.update(pred=p["dev"]["pred"], pred_stride=p["stride"], pred_off=p["off_dev"])
        if chroma and "pred_c" in outs.planes:
            p = outs.planes["pred_c"]
            it.update(pred_cb=p["dev"]["pred_cb"], pred_cr=p["dev"]["pred_cr"], pred_cstride=p["stride"],
                      pred_coff=p["off_dev"])
        return it


def run(prims, depth, items):
    import torch

    from src.x265_amd.native import inter_cost_batches

    prims.inter_costs(depth, inter_cost_batches(items))
    torch.cuda.synchronize()


def check(outs, got, want, where, j0=0, j1=None):
    """every output that was asked for equals the expected values of CUs j0..j1, the prediction planes as a
    whole (so nothing outside a live CU's footprint changed)"""
    j1 = len(want["best"]) if j1 is None else j1
    for k in ("sad", "cost", "best"):
        if k in got:
            w = want[k][j0:j1]
            bad = [j for j in range(len(w)) if not np.array_equal(got[k][j], w[j])]
            assert not bad, f"{where}: {k} differs at CUs {bad[:8]}: got {got[k][bad[0]]} want {w[bad[0]]}"
    live = want["best"]["cand"][j0:j1] >= 0
    for nm in ("pred", "pred_cb", "pred_cr"):
        if nm in got:
            w = outs.want_plane(nm, want[nm][j0:j1], live)
            diff = np.nonzero(got[nm] != w)[0]
            assert not len(diff), f"{where}: {nm} differs at {len(diff)} elements, first at {int(diff[0])}"


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("log2", SIZES)
def test_gpu_batch_matches_oracle_chain(prims, oracle_libs, depth, log2):
    """13 CUs x 5 slots with chroma, every content class, all outputs including the three prediction planes"""
    want = icc.expected(log2, depth)
    db = DeviceBatch(log2, depth)
    outs = Outputs(db.n, db.K, 1 << log2, depth)
    run(prims, depth, [db.item(outs)])
    got, intact = outs.read()
    check(outs, got, want, f"log2 {log2} depth {depth}")
    assert intact, "writes outside the outputs"
    assert not got["best"]["reserved"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
def test_gpu_luma_only(prims, oracle_libs, depth):
    """chroma NULL (m_bChromaSa8d off) at every size: luma distortions, and only the luma prediction"""
    for log2 in SIZES:
        want = icc.expected(log2, depth, chroma=False)
        db = DeviceBatch(log2, depth)
        outs = Outputs(db.n, db.K, 1 << log2, depth, ("sad", "cost", "best", "pred"))
        run(prims, depth, [db.item(outs, chroma=False)])
        got, intact = outs.read()
        check(outs, got, want, f"luma only, log2 {log2} depth {depth}")
        assert intact


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
def test_gpu_output_subsets(prims, oracle_libs, depth):
    """sad only with bits = NULL, best only, and pred only, at every size"""
    for log2 in SIZES:
        want = icc.expected(log2, depth)
        db = DeviceBatch(log2, depth)
        N = 1 << log2
        for which, rd in ((("sad",), False), (("best",), True), (("pred", "pred_c"), True)):
            outs = Outputs(db.n, db.K, N, depth, which)
            run(prims, depth, [db.item(outs, rd=rd)])
            got, intact = outs.read()
            check(outs, got, want, f"log2 {log2} depth {depth} subset {which}")
            assert intact


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
def test_gpu_mixed_sizes_in_one_call(prims, oracle_libs, depth):
    """count = 3 (8x8, 16x16, 64x64) in one call equals three single calls, and both equal the oracle chain"""
    sizes = (3, 4, 6)
    dbs = [DeviceBatch(l, depth) for l in sizes]
    mixed = [Outputs(db.n, db.K, 1 << db.log2, depth) for db in dbs]
    single = [Outputs(db.n, db.K, 1 << db.log2, depth) for db in dbs]
    run(prims, depth, [db.item(o) for db, o in zip(dbs, mixed)])
    for db, o in zip(dbs, single):
        run(prims, depth, [db.item(o)])
    for l, m, s in zip(sizes, mixed, single):
        gm, im = m.read()
        gs, i_s = s.read()
        for k in gm:
            assert np.array_equal(gm[k], gs[k]), f"log2 {l}: {k} of the mixed call differs from the single call"
        check(m, gm, icc.expected(l, depth), f"mixed log2 {l} depth {depth}")
        assert im and i_s


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
def test_gpu_single_cus_in_guarded_slots(prims, oracle_libs, depth):
    """n = 1 calls, each CU's outputs in buffers of its own with sentinel padding on both sides"""
    for log2 in SIZES:
        want = icc.expected(log2, depth)
        db = DeviceBatch(log2, depth)
        for j in (icc.FLAT, icc.COLS, icc.TWIN, icc.ALLDEAD, 12):
            outs = Outputs(1, db.K, 1 << log2, depth)
            run(prims, depth, [db.item(outs, j0=j, j1=j + 1)])
            got, intact = outs.read()
            check(outs, got, want, f"n = 1, log2 {log2} depth {depth} CU {j}", j, j + 1)
            assert intact, f"log2 {log2} CU {j}: sentinel padding changed"


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("K", [1, 2])
def test_gpu_one_and_two_slots(prims, oracle_libs, depth, K):
    """K = 1 (plain fused motion compensation: the one candidate's prediction is the output) and the K = 2
    bidir shape (bi with the two best MVs, bi with both MVs zero), at every size"""
    for log2 in SIZES:
        want = icc.expected(log2, depth, True, K)
        db = DeviceBatch(log2, depth, K)
        outs = Outputs(db.n, K, 1 << log2, depth)
        run(prims, depth, [db.item(outs)])
        got, intact = outs.read()
        check(outs, got, want, f"K {K} log2 {log2} depth {depth}")
        assert intact


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
def test_gpu_all_slots_dead(prims, oracle_libs, depth):
    """the CU with dir 0 in every slot: cand -1, cost INT64_MAX, all-ones sad / cost, prediction untouched"""
    for log2 in SIZES:
        db = DeviceBatch(log2, depth)
        outs = Outputs(1, db.K, 1 << log2, depth)
        j = icc.ALLDEAD
        run(prims, depth, [db.item(outs, j0=j, j1=j + 1)])
        got, intact = outs.read()
        assert intact
        assert got["best"]["cand"][0] == -1 and got["best"]["cost"][0] == icc.NO_COST
        assert not got["best"]["sad"][0] and not got["best"]["bits"][0] and not got["best"]["reserved"][0]
        assert (got["sad"] == icc.DEAD_SAD).all() and (got["cost"] == icc.DEAD_COST).all()
        for nm, p in (("pred", "pred"), ("pred_cb", "pred_c"), ("pred_cr", "pred_c")):
            assert np.array_equal(got[nm], outs.planes[p]["fill"]), f"log2 {log2}: {nm} of a dead CU was written"
