"""x265amd_intra_costs: the fused intra mode decision (35 predictions + SA8D per block, cost and winner)
against the oracle chain of tests/intra_cost_cases.py — exact equality on every element."""
import ctypes

import numpy as np
import pytest

import intra_cost_cases as icc

SIZES = (2, 3, 4, 5, 6)
EINVAL = 1000


# ---------------------------------------------------------------- CPU: the ABI surface (no device)
@pytest.fixture(scope="module")
def lib(native_lib):
    lib = ctypes.CDLL(native_lib)
    lib.x265amd_sizeof.argtypes = [ctypes.c_char_p]
    return lib


def test_entry_is_exported(lib):
    assert hasattr(lib, "x265amd_intra_costs")


def test_descriptor_sizes_match(lib):
    from src.x265_amd.native import IntraBest, IntraCostBatch

    assert lib.x265amd_sizeof(b"x265amd_intra_best") == ctypes.sizeof(IntraBest) == icc.BEST_DTYPE.itemsize
    assert lib.x265amd_sizeof(b"x265amd_intra_cost_batch") == ctypes.sizeof(IntraCostBatch) > 0


def _desc(**kw):
    """a descriptor whose pointers are small non-null integers: validation must reject before any is used"""
    from src.x265_amd.native import IntraCostBatch

    d = dict(log2_size=3, n=1, strong_smoothing=0, fenc=8, fenc_stride=64, fenc_off=8, nb=8, nb_off=8, mpm=8, bits=8,
             lambda_=8, sad=8, cost=8, best=8)
    d.update(kw)
    return (IntraCostBatch * 1)(IntraCostBatch(**d))


INVALID = [
    ("depth", 9, 1, {}),
    ("log2_size below", 8, 1, dict(log2_size=1)),
    ("log2_size above", 8, 1, dict(log2_size=7)),
    ("n < 0", 8, 1, dict(n=-1)),
    ("count < 0", 8, -1, {}),
    ("fenc NULL", 8, 1, dict(fenc=None)),
    ("nb NULL", 8, 1, dict(nb=None)),
    ("fenc_off NULL", 8, 1, dict(fenc_off=None)),
    ("nb_off NULL", 8, 1, dict(nb_off=None)),
    ("cost without mpm", 8, 1, dict(mpm=None, best=None)),
    ("best without bits", 8, 1, dict(bits=None, cost=None)),
    ("best without lambda", 8, 1, dict(lambda_=None, cost=None)),
    ("no output", 8, 1, dict(sad=None, cost=None, best=None)),
]


@pytest.mark.parametrize("what,depth,count,kw", INVALID, ids=[c[0].replace(" ", "_") for c in INVALID])
def test_invalid_calls_rejected_without_launch(lib, what, depth, count, kw):
    assert lib.x265amd_intra_costs(depth, count, _desc(**kw), None) == EINVAL, what


def test_second_batch_invalid_rejects_whole_call(lib):
    from src.x265_amd.native import IntraCostBatch

    arr = (IntraCostBatch * 2)(IntraCostBatch(3, 0), IntraCostBatch(9, 1, 0, 8, 64, 8, 8, 8, 8, 8, 8, 8, 8, 8))
    assert lib.x265amd_intra_costs(8, 2, arr, None) == EINVAL


def test_empty_calls_are_noops(lib):
    from src.x265_amd.native import IntraCostBatch

    assert lib.x265amd_intra_costs(8, 0, None, None) == 0
    assert lib.x265amd_intra_costs(10, 1, (IntraCostBatch * 1)(IntraCostBatch(4, 0)), None) == 0


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def prims(native_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a gfx950 device"
    from src.x265_amd import Primitives

    return Primitives(device=0)


SENTINEL = 0x5A
PAD = 64                         # bytes of sentinel on each side of an output


class Outputs:
    """sad / cost / best device buffers for n jobs, each between PAD sentinel bytes"""

    SIZES = dict(sad=35 * 4, cost=35 * 8, best=24)

    def __init__(self, n, which=("sad", "cost", "best")):
        import torch

        self.n = n
        self.box = {k: torch.full((n * self.SIZES[k] + 2 * PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
                    for k in which}

    def get(self, k):
        return self.box[k][PAD:] if k in self.box else None

    def read(self):
        """(outputs as numpy, sentinel padding intact)"""
        out, ok = {}, True
        for k, box in self.box.items():
            h = box.cpu().numpy()
            ok = ok and (h[:PAD] == SENTINEL).all() and (h[-PAD:] == SENTINEL).all()
            body = h[PAD:-PAD]
            out[k] = (body.view(np.int32).reshape(self.n, 35) if k == "sad" else
                      body.view(np.uint64).reshape(self.n, 35) if k == "cost" else body.view(icc.BEST_DTYPE))
        return out, bool(ok)


class DeviceBatch:
    """one batch's inputs on the device; item() makes the intra_cost_batches tuple for a job range"""

    def __init__(self, log2, depth, n=icc.N_JOBS):
        import torch

        b = icc.make_batch(log2, depth, n)
        self.log2, self.depth, self.n, self.fs = log2, depth, n, b["fenc_stride"]
        dev = lambda a: torch.from_numpy(np.array(a)).to("cuda")          # (a copy: the cached cases are read-only)
        self.fenc, self.foff, self.nb, self.nboff = dev(b["fenc"]), dev(b["fenc_off"]), dev(b["nb"]), dev(b["nb_off"])
        self.mpm = dev(icc.mpm_modes(log2, depth, n).reshape(-1))
        self.bits = dev(b["bits"].view(np.int32).reshape(-1))
        self.lam = dev(b["lam"].view(np.int32))

    def item(self, outs, strong=0, rd=True, j0=0, j1=None):
        j1 = self.n if j1 is None else j1
        return (self.log2, strong, self.fenc, self.fs, self.foff[j0:j1], self.nb, self.nboff[j0:j1],
                self.mpm[3 * j0:] if rd else None, self.bits[4 * j0:] if rd else None, self.lam[j0:] if rd else None,
                outs.get("sad"), outs.get("cost"), outs.get("best"))


def run(prims, depth, items):
    import torch

    from src.x265_amd.native import intra_cost_batches

    prims.intra_costs(depth, intra_cost_batches(items))
    torch.cuda.synchronize()


def check(got, want, where):
    sad, cost, best = want
    for k, w in (("sad", sad), ("cost", cost), ("best", best)):
        if k in got:
            bad = [j for j in range(len(w)) if not np.array_equal(got[k][j], w[j])]
            assert not bad, f"{where}: {k} differs at jobs {bad[:8]}: got {got[k][bad[0]]} want {w[bad[0]]}"


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("log2,strong", [(2, 0), (3, 0), (4, 0), (5, 0), (5, 1), (6, 0)])
def test_gpu_batch_matches_oracle_chain(prims, oracle_libs, depth, log2, strong):
    """37 jobs of one size, every content class, all three outputs; the 32x32 batch with strong smoothing
    off and on"""
    want = icc.expected(log2, depth, strong)
    db, outs = DeviceBatch(log2, depth), Outputs(icc.N_JOBS)
    run(prims, depth, [db.item(outs, strong)])
    got, intact = outs.read()
    check(got, want, f"log2 {log2} depth {depth} strong {strong}")
    assert intact, "writes outside the outputs"
    assert not got["best"]["reserved"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
def test_gpu_output_subsets(prims, oracle_libs, depth):
    """sad only with mpm = NULL, and best only, at every size"""
    for log2 in SIZES:
        want = icc.expected(log2, depth, 0)
        db = DeviceBatch(log2, depth)
        o_sad, o_best = Outputs(icc.N_JOBS, ("sad",)), Outputs(icc.N_JOBS, ("best",))
        run(prims, depth, [db.item(o_sad, rd=False)])
        run(prims, depth, [db.item(o_best)])
        for o in (o_sad, o_best):
            got, intact = o.read()
            check(got, want, f"log2 {log2} depth {depth} subset {list(got)}")
            assert intact


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
def test_gpu_mixed_sizes_in_one_call(prims, oracle_libs, depth):
    """count = 3 (4x4, 16x16, 64x64) in one call equals three single calls, and both equal the oracle chain"""
    sizes = (2, 4, 6)
    dbs = [DeviceBatch(l, depth) for l in sizes]
    mixed = [Outputs(icc.N_JOBS) for _ in sizes]
    single = [Outputs(icc.N_JOBS) for _ in sizes]
    run(prims, depth, [db.item(o) for db, o in zip(dbs, mixed)])
    for db, o in zip(dbs, single):
        run(prims, depth, [db.item(o)])
    for l, m, s in zip(sizes, mixed, single):
        gm, im = m.read()
        gs, i_s = s.read()
        for k in gm:
            assert np.array_equal(gm[k], gs[k]), f"log2 {l}: {k} of the mixed call differs from the single call"
        check(gm, icc.expected(l, depth, 0), f"mixed log2 {l} depth {depth}")
        assert im and i_s


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10])
def test_gpu_single_jobs_in_guarded_slots(prims, oracle_libs, depth):
    """n = 1 calls, each job's outputs in a slot of its own with sentinel padding on both sides: the slot
    holds the job's expected values and no padding byte changes"""
    for log2 in SIZES:
        strong = 1 if log2 == 5 else 0
        want = icc.expected(log2, depth, strong)
        db = DeviceBatch(log2, depth)
        jobs = (0, 1, 4, 7, 36)
        slots = [Outputs(1) for _ in jobs]
        for j, o in zip(jobs, slots):
            run(prims, depth, [db.item(o, strong, j0=j, j1=j + 1)])
        for j, o in zip(jobs, slots):
            got, intact = o.read()
            check(got, tuple(w[j:j + 1] for w in want), f"n = 1, log2 {log2} depth {depth} job {j}")
            assert intact, f"log2 {log2} job {j}: sentinel padding changed"
