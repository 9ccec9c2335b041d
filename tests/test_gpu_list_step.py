"""The tensor-list outer step (edt_outer_step_list) at the shapes where its host-built table and
its per-chunk search can go wrong (needs an MI355X).

Bar, everywhere: bit for bit against `oracle.outer_step` on the same values concatenated flat
(the tail form: against `ops.outer_step(..., tail_bits=)` on the device). No tolerances.

Every operand lives in a guarded layout: one device buffer per operand (theta, momentum, each
worker), the T tensors laid into it as views, gaps of at least 8 elements between and around them
filled with a quiet NaN of a recognisable payload. After a step every gap must still hold those
bits and the worker buffers must be unchanged, so a store or a skipped element at a tensor's edge
fails the test where separate allocations would hide it in allocator slack.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests.golden_data import bits

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
REGIMES = [(F32, F32), (F32, BF16), (BF16, BF16)]
# (has_momentum, lr, mu, nesterov), as test_outer_step_list_vs_oracle
HYPERS = [(False, 0.7, 0.9, True), (True, 0.7, 0.9, True), (True, 0.5, 0.8, False), (False, 1.0, 0.0, False)]
HYPERS2 = [(True, 0.7, 0.9, True), (False, 1.0, 0.0, False)]

CHUNK = 4096                                  # kListChunk: 256 threads x 8 elements x EDT_LIST_ITERS (2)
GAP = 8                                       # elements, a multiple of 16 bytes in both dtypes
SENTINEL = {F32: 0x7FC0BEEF, BF16: 0x7FED}    # quiet NaNs
INT = {F32: torch.int32, BF16: torch.int16}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from evolutionarydistributedtraining_amd import ops as o
    return o


# ------------------------------------------------------------------------------------------
# the guarded layout

class Layout:
    """Where T tensors of sizes `numels` sit in one buffer of `dtype`: tensor t starts on a 16-byte
    boundary plus shift[t] elements, at least GAP elements after the end of tensor t - 1."""

    def __init__(self, numels, dtype, shift=None):
        shift = shift or {}
        al = 16 // torch.empty((), dtype=dtype).element_size()
        starts, pos, end = [], GAP, 0
        for t, n in enumerate(numels):
            s = -(-pos // al) * al + shift.get(t, 0)
            assert s - end >= GAP
            starts.append(s)
            end = s + n
            pos = end + GAP
        self.dtype, self.total, self.spans = dtype, end + GAP, [(s, s + n) for s, n in zip(starts, numels)]
        self.starts = np.asarray(starts, dtype=np.int64)
        nn = np.asarray(numels, dtype=np.int64)
        assert ((self.starts % al) == [shift.get(t, 0) for t in range(len(numels))]).all()
        offs = np.concatenate([[0], np.cumsum(nn)])[:-1]
        # buffer position of every element of the flat concatenation
        self.idx = torch.from_numpy(np.arange(int(nn.sum()), dtype=np.int64) + np.repeat(self.starts - offs, nn))
        self.gap = torch.ones(self.total, dtype=torch.bool)
        self.gap[self.idx] = False
        assert int(self.gap.sum()) >= GAP * (len(numels) + 1)


class Guarded:
    """One operand: `values` (flat, CPU) laid out by `lay` in one device buffer of sentinels."""

    def __init__(self, values, lay, dev):
        assert values.dtype == lay.dtype and values.numel() == lay.idx.numel()
        self.lay, self.values = lay, values
        self.host0 = torch.full((lay.total,), SENTINEL[lay.dtype], dtype=INT[lay.dtype])
        self.host0[lay.idx] = bits(values)
        self.buf = self.host0.to(dev).view(lay.dtype)
        assert self.buf.data_ptr() % 16 == 0
        self.views = [self.buf[a:b] for a, b in lay.spans]

    def reset(self):
        self.buf.copy_(self.host0.view(self.lay.dtype))

    def read(self):
        return self.buf.view(INT[self.lay.dtype]).cpu()

    def check(self, want, what):
        """Buffer == `want` (flat values, None: the initial ones) inside the tensors, sentinels outside."""
        got = self.read()
        if want is None:
            assert torch.equal(got, self.host0), f"{what}: buffer changed"
            return
        bad = got[self.lay.gap] != SENTINEL[self.lay.dtype]
        assert not bad.any(), f"{what}: {int(bad.sum())} guard elements overwritten"
        assert torch.equal(got[self.lay.idx], bits(want)), f"{what}: values differ from the reference's"


def _rand_case(n, K, gdt, wdt, seed):
    g = torch.Generator().manual_seed(seed)
    theta = (torch.randn(n, generator=g) * 0.02).to(gdt)
    workers = [(theta.float() + torch.randn(n, generator=g) * 1e-3).to(wdt) for _ in range(K)]
    mom = (torch.randn(n, generator=g) * 1e-3).to(gdt)
    return theta, workers, mom


class Case:
    """A guarded tensor list with random values. shifts: {operand: {t: elements}} moves single
    pointers off their 16-byte boundary; operand is "theta", "mom" or a worker index."""

    def __init__(self, dev, numels, K, gdt, wdt, seed, shifts=None):
        shifts = shifts or {}
        self.numels, self.K, self.n = list(numels), K, sum(numels)
        theta, workers, mom = _rand_case(self.n, K, gdt, wdt, seed)
        self.theta = Guarded(theta, Layout(numels, gdt, shifts.get("theta")), dev)
        self.mom = Guarded(mom, Layout(numels, gdt, shifts.get("mom")), dev)
        plain = Layout(numels, wdt)
        self.workers = [Guarded(w, Layout(numels, wdt, shifts[k]) if k in shifts else plain, dev)
                        for k, w in enumerate(workers)]

    def reset(self):
        self.theta.reset()
        self.mom.reset()

    def operands(self, mu, pass_momenta=None):
        pass_momenta = bool(mu) if pass_momenta is None else pass_momenta
        return self.theta.views, [w.views for w in self.workers], self.mom.views if pass_momenta else None

    def step(self, ops, hyper, pass_momenta=None, tails=None):
        has, lr, mu, nest = hyper
        th, ws, ms = self.operands(mu, pass_momenta)
        ops.outer_step_list(th, ws, ms, has, lr, mu, nest, tails=tails)

    def check(self, oracle, hyper):
        has, lr, mu, nest = hyper
        th, m = self.theta.values.clone(), self.mom.values.clone()
        if self.n:
            oracle.outer_step(th, [w.values for w in self.workers], m if mu else None, has, lr, mu, nest)
        self.theta.check(th, f"theta {hyper}")
        self.mom.check(m if mu else None, f"momentum {hyper}")
        for k, w in enumerate(self.workers):
            w.check(None, f"worker {k} {hyper}")

    def run(self, oracle, ops, hypers, pass_momenta=None):
        for hyper in hypers:
            self.reset()
            self.step(ops, hyper, pass_momenta)
            self.check(oracle, hyper)


# ------------------------------------------------------------------------------------------
# 1. chunk and tile edges

EDGE_SIZES = [2047, 2048, 2049, 4095, 4096, 4097, 6143, 6144, 6145, 8191, 8192, 8193, 1, 0, 12289]


@pytest.mark.parametrize("gdt,wdt", REGIMES)
@pytest.mark.parametrize("K", [2, 3])
def test_chunk_and_tile_edges(oracle, dev, ops, gdt, wdt, K):
    """Sizes next to the 2048-element tile, the 4096-element chunk and a chunk plus a tile: where
    vend, c1 and the split-halves tile mapping of outer_list_chunk change."""
    Case(dev, EDGE_SIZES, K, gdt, wdt, seed=100 + K).run(oracle, ops, HYPERS)


# ------------------------------------------------------------------------------------------
# 2. long lists across the LDS boundary (kListLdsMaxTensors = 8191)

# 0 twice in a row, 1, 7, 8, 9, one-chunk (2049) and two-chunk (4097) tensors; ~3.4 M elements at T = 8192
LONG_PATTERN = [0, 1, 7, 8, 9, 2049, 4097, 0, 0, 3, 8, 1, 9, 7, 16]


@pytest.mark.parametrize("gdt,wdt", REGIMES)
@pytest.mark.parametrize("T", [8190, 8191, 8192, 8193])
def test_long_list_across_lds_boundary(oracle, dev, ops, gdt, wdt, T):
    """T <= 8191 searches the prefix sums staged in LDS (T = 8191: exactly 64 KiB of dynamic LDS),
    T > 8191 the global table; every search outcome (equal neighbouring prefixes, one- and
    two-chunk tensors) occurs up to the highest t."""
    numels = [LONG_PATTERN[t % len(LONG_PATTERN)] for t in range(T)]
    Case(dev, numels, 2, gdt, wdt, seed=T).run(oracle, ops, HYPERS2)


def _tiny_sizes(T, mul=7):
    return [1 + (t * mul) % 9 for t in range(T)]


@pytest.mark.parametrize("gdt,wdt", REGIMES)
def test_long_list_most_workers(oracle, dev, ops, gdt, wdt):
    """T = 8193, K = 64, tensors of 1 to 9 elements: the largest table, w[k * T + t] at both extremes."""
    Case(dev, _tiny_sizes(8193), 64, gdt, wdt, seed=64).run(oracle, ops, HYPERS2)


# ------------------------------------------------------------------------------------------
# 3. every K body: the K = 2 and K = 4 specialisations, the generic loop's unroll-by-4 remainders
# 2 and 3, the maximum K

RAGGED = [5, 3 * CHUNK + 77, 0, 2048, 2051, 4097, 1, 8, 6143, 31]


@pytest.mark.parametrize("gdt,wdt", REGIMES)
@pytest.mark.parametrize("K", [2, 4, 6, 7, 64])
def test_every_k_body(oracle, dev, ops, gdt, wdt, K):
    """A ragged list with an empty tensor, a tensor of three chunks and a remainder and one tensor
    (2051 elements) whose every operand starts one element off a 16-byte boundary."""
    off = {4: 1}
    shifts = {"theta": off, "mom": off, **{k: off for k in range(K)}}
    Case(dev, RAGGED, K, gdt, wdt, seed=300 + K, shifts=shifts).run(oracle, ops, HYPERS)


# ------------------------------------------------------------------------------------------
# 4. one pointer of one tensor off alignment

MISALIGN_SIZES = [2 * CHUNK + 5, 2 * CHUNK + 2049, 2 * CHUNK + 77, 3 * CHUNK + 1, 2 * CHUNK + 4095]


@pytest.mark.parametrize("gdt,wdt", REGIMES)
@pytest.mark.parametrize("which", ["theta", "mom", 0, 2])
def test_single_operand_misaligned(oracle, dev, ops, gdt, wdt, which):
    """Exactly one of tensor 2's 2 + K pointers is one element off a 16-byte boundary, its aligned
    neighbours cross chunks on both sides: the tensor takes the scalar body, the others do not
    move. With mu = 0 the momentum does not count, whether it is passed or not."""
    c = Case(dev, MISALIGN_SIZES, 3, gdt, wdt, seed=400, shifts={which: {2: 1}})
    moved = {"theta": c.theta, "mom": c.mom}.get(which) or c.workers[which]
    es = moved.buf.element_size()
    assert [v.data_ptr() % 16 for v in moved.views] == [0, 0, es, 0, 0]
    c.run(oracle, ops, HYPERS)
    c.run(oracle, ops, [HYPERS[3]], pass_momenta=True)


# ------------------------------------------------------------------------------------------
# 5. empty tensors at the edges, the smallest lists

@pytest.mark.parametrize("gdt,wdt", REGIMES)
@pytest.mark.parametrize("numels", [[4097, 9, 0, 0, 0, 0], [0, 0, 0, 0, 9, 4097], [0, 0, 0, 0, 0], [1], [4096]],
                         ids=["trailing", "leading", "all_empty", "one_element", "one_chunk"])
def test_empty_edges(oracle, dev, ops, gdt, wdt, numels):
    """prefix[T-4] == ... == prefix[T], prefix[0] == ... == prefix[4], no chunk at all (no launch,
    nothing touched), a single element, a single tensor of exactly one chunk."""
    c = Case(dev, numels, 3, gdt, wdt, seed=500 + len(numels))
    c.run(oracle, ops, HYPERS)
    if not c.n:
        c.run(oracle, ops, HYPERS2, pass_momenta=True)


# ------------------------------------------------------------------------------------------
# 6. two steps back to back: the host table of the first must not be the second's

def _abi_call(c, hyper):
    """The edt_outer_step_list call of ops.outer_step_list on case c with every argument built ahead,
    so that two of them run with nothing but the two C calls between the uploads."""
    from evolutionarydistributedtraining_amd import _lib as L
    lib = L.lib()
    has, lr, mu, nest = hyper
    th, ws, ms = c.operands(mu)
    T, K = len(th), len(ws)
    P_ = ctypes.c_void_p
    th_arr = (P_ * T)(*[t.data_ptr() for t in th])
    w_arr = (P_ * (K * T))(*[t.data_ptr() for w in ws for t in w])
    m_arr = (P_ * T)(*[t.data_ptr() for t in ms]) if ms is not None else None
    numel = (ctypes.c_uint64 * T)(*c.numels)
    nbytes = lib.edt_outer_list_workspace_bytes(T, K)
    work = torch.empty(nbytes, dtype=torch.uint8, device=th[0].device)
    gdt, wdt, stream = L.dtype_code(th[0]), L.dtype_code(ws[0][0]), L.stream_ptr(th[0].device)

    def call():
        L.check(lib.edt_outer_step_list(th_arr, gdt, w_arr, wdt, K, m_arr, int(has), numel, T, float(lr),
                                        float(mu), int(nest), L.ptr(work), nbytes, stream), "edt_outer_step_list")
    return call


_PAIRS = {}


def _pair(dev, size, gdt, wdt):
    """Two lists of different T, buffers and sizes at equal t, built once for both orders."""
    key = (size, gdt, wdt)
    if key not in _PAIRS:
        if size == "small":             # tables of a few tens of KB
            K = 8
            a = [LONG_PATTERN[t % len(LONG_PATTERN)] for t in range(300)]
            b = [x + 3 for x in a[:283]]
        else:                           # about 4.5 MB each
            K = 64
            a = _tiny_sizes(8193)
            b = [x % 9 + 1 for x in a[:8000]]
        assert all(x != y for x, y in zip(a, b))
        _PAIRS[key] = (Case(dev, a, K, gdt, wdt, seed=600), Case(dev, b, K, gdt, wdt, seed=601))
    return _PAIRS[key]


@pytest.fixture(scope="module", autouse=True)
def _drop_pairs():
    yield
    _PAIRS.clear()


@pytest.mark.parametrize("gdt,wdt", REGIMES)
@pytest.mark.parametrize("order", ["ab", "ba"])
@pytest.mark.parametrize("via", ["ops", "abi"])
@pytest.mark.parametrize("size", ["small", "large"])
def test_back_to_back_steps(oracle, dev, ops, gdt, wdt, size, via, order):
    """Two list steps with different tables on one host thread and one stream, no host wait between
    them: each must run with its own table, although the second call rebuilds the thread's host
    table right after the first has handed it to hipMemcpyAsync. via="abi" calls the C entry with
    arguments built ahead, so nothing but the second call's own table building lies between the
    two uploads. Run once; this is no race hunt."""
    pair = _pair(dev, size, gdt, wdt)
    hypers = [(True, 0.7, 0.9, True), (True, 0.5, 0.8, False)]
    todo = list(zip(pair, hypers))
    if order == "ba":
        todo.reverse()
    for c in pair:
        c.reset()
    if via == "abi":
        calls = [_abi_call(c, h) for c, h in todo]
        torch.cuda.synchronize()            # the resets are done; from here on no host wait
        calls[0]()
        calls[1]()
    else:
        torch.cuda.synchronize()
        todo[0][0].step(ops, todo[0][1])
        todo[1][0].step(ops, todo[1][1])
    for c, h in todo:
        c.check(oracle, h)


# ------------------------------------------------------------------------------------------
# 7. the tail form: tail_off is the sixth array of the table, behind w[K * T]

@pytest.mark.parametrize("T,K", [(8192, 5), (9, 8)])
def test_tail_form_at_other_table_shapes(dev, ops, T, K):
    """edt_outer_step_list_tail == edt_outer_step_tail over the same values packed flat, bit for
    bit, two generations, all-bf16, at table shapes that move tail_off[] (its address depends on
    K and T) and on the global-table search."""
    from evolutionarydistributedtraining_amd.torchcompat import torch_cpu_tail_bits, torch_cpu_tail_bits_per_tensor
    pattern = [33, 5, 257, 4097, 0, 31]
    numels = [pattern[t % len(pattern)] for t in range(T)]
    c = Case(dev, numels, K, BF16, BF16, seed=700 + T)
    flat_theta = c.theta.values.to(dev)
    flat_mom = c.mom.values.to(dev)
    flat_workers = [w.values.to(dev) for w in c.workers]
    tails = torch_cpu_tail_bits_per_tensor(numels, device=dev)
    flat_bits = torch_cpu_tail_bits(numels, device=dev)
    for gen in range(2):
        hyper = (gen > 0, 0.7, 0.9, True)
        c.step(ops, hyper, tails=tails)
        ops.outer_step(flat_theta, flat_workers, flat_mom, *hyper, tail_bits=flat_bits)
        c.theta.check(flat_theta.cpu(), f"theta, generation {gen}")
        c.mom.check(flat_mom.cpu(), f"momentum, generation {gen}")
    for k, w in enumerate(c.workers):
        w.check(None, f"worker {k}")
