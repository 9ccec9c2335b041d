"""Stochastic rounding of the quantized exchange (EDT_ROUND_STOCHASTIC) without a GPU: Philox4x32's
known answers, the properties of the numpy definition (tests/sr_reference.py), the host-side
validation of the two new C-ABI entries (edt_delta_partial_q_sr, edt_sgd_delta_sum_q_sr), the
option handling of ShardedOuterSync and its schedule on virtual ranks through the kernels= seam.
The reference project quantizes nothing (its workers exchange checkpoints on disk,
EDT_LM/diloco.py:231-235, 302-308); the GPU form is tests/test_gpu_sr.py."""
import ctypes

import numpy as np
import pytest
import torch

from tests import gather_q_reference as G
from tests import quant_reference as Q
from tests import sr_reference as S
from tests.virtual_schedules import bits, population

FMTS = ["mxfp8", "mxfp4"]
MAXV = {"mxfp8": 448.0, "mxfp4": 6.0}
QB = {"mxfp8": 1 + 1 / 32, "mxfp4": 1 / 2 + 1 / 32}


# ---------------------------------------------------------------------------------------------
# the generator

KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        "d16cfe09 94fdcceb 5001e420 24126ea1")]


def test_philox_known_answers():
    for ctr, key, want in KAT:
        got = S.philox4x32(np.array(ctr), np.array(key), rounds=10)
        assert " ".join(f"{int(w):08x}" for w in got) == want
    assert S.PHILOX_ROUNDS == 10                 # what ships; the header's constant is the one the kernels use
    # vectorised over counters, and the element -> (word, half) map of random_bits
    ctrs = np.array([k[0] for k in KAT[:1]] * 3)
    assert np.array_equal(S.philox4x32(ctrs, np.array([0, 0])), np.tile(S.philox4x32(ctrs[0], np.array([0, 0])), (3, 1)))
    r = S.random_bits(0, 0, 0, 8)
    assert [int(x) for x in r] == [0xe8d5, 0x6627, 0xc58d, 0xe169, 0xac4c, 0xbc57, 0xdbd8, 0x9b00]
    seed, step, stream = 0x299f31d0a4093822, 0x13198a2e, 0x03707344
    g = (0x85a308d3 << 32) | 0x243f6a88
    r = S.random_bits(seed, step | (7 << 32), stream, 8, elem_base=8 * g)          # step: low 32 bits only
    assert [int(x) for x in r] == [0xfe09, 0xd16c, 0xcceb, 0x94fd, 0xe420, 0x5001, 0x6ea1, 0x2412]
    # bits depend on the global element index, not on where a call starts
    a = S.random_bits(5, 9, 3, 4096)
    assert np.array_equal(a[2048:], S.random_bits(5, 9, 3, 2048, elem_base=2048))
    assert not np.array_equal(a, S.random_bits(5, 10, 3, 4096)) and not np.array_equal(a, S.random_bits(5, 9, 4, 4096))
    assert not np.array_equal(a, S.random_bits(6, 9, 3, 4096))


# ---------------------------------------------------------------------------------------------
# the definition's properties

def _data(fmt, n=32 * 512, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * np.exp2(rng.integers(-30, 30, n))).astype(np.float32)


@pytest.mark.parametrize("fmt", FMTS)
def test_a_value_on_the_grid_never_moves(fmt):
    grid = Q.finite_grid(fmt)
    reps = -(-32 // len(grid))
    blk = np.resize(np.concatenate([grid] * reps), 32 * ((len(grid) * reps + 31) // 32))     # every block holds the maximum
    blk = blk.reshape(-1, 32)
    blk[:, 0] = grid[-1]
    x = np.concatenate([(blk * 2.0 ** s * sg).reshape(-1) for s in (-20, 0, 7) for sg in (1, -1)]).astype(np.float32)
    rng = np.random.default_rng(1)
    for r16 in (np.zeros(x.size), np.full(x.size, 0xffff), np.ones(x.size), rng.integers(0, 1 << 16, x.size)):
        codes, scales = S.quantize_sr(x, fmt, r16.astype(np.uint32))
        assert np.array_equal(Q.dequantize(codes, scales, fmt).view(np.int32), x.view(np.int32))


@pytest.mark.parametrize("fmt", FMTS)
def test_every_result_is_one_of_the_two_neighbours_and_nothing_saturates(fmt):
    x = _data(fmt)
    step = S.grid_step(x, fmt)
    rng = np.random.default_rng(2)
    lo = hi = None
    for r16 in (np.zeros(x.size), np.full(x.size, 0xffff), rng.integers(0, 1 << 16, x.size)):
        codes, scales = S.quantize_sr(x, fmt, r16.astype(np.uint32))
        assert scales.max() <= 253
        d = Q.dequantize(codes, scales, fmt).astype(np.float64)
        assert (np.abs(d - x) < step).all()
        assert np.array_equal(np.signbit(d), np.signbit(x))
        if lo is None:
            # r16 = 0: up whenever f16 > 0, i.e. unless the value lies within 2^-16 of a step above
            # its lower neighbour — away from zero, the block maximum included, so nothing was
            # clamped; r16 = 0xffff: never up — toward zero
            lo = d
            assert (np.abs(d) - np.abs(x) > -step * 2.0 ** -16).all()
        elif hi is None:
            hi = d
            assert (np.abs(d) <= np.abs(x)).all()
            assert (np.abs(lo - hi) <= step).all() and (np.abs(lo - hi)[lo != hi] == step[lo != hi]).all()
        else:
            assert ((d == lo) | (d == hi)).all()


@pytest.mark.parametrize("fmt", FMTS)
def test_the_scale_is_bumped_exactly_when_the_maximum_would_saturate(fmt):
    m = MAXV[fmt]
    emax = Q.FORMATS[fmt]["emax"]
    top = 2.0 ** (emax + 1)
    rng = np.random.default_rng(3)
    for s in (-40, -3, 0, 11):
        for amax, bumped in [(m, False), (np.nextafter(np.float32(m), np.float32(np.inf)), True), ((m + top) / 2, True),
                             (np.nextafter(np.float32(top), np.float32(0)), True), (m * 0.75, False), (top / 2, False)]:
            blk = (rng.uniform(-1, 1, 32) * amax * 0.9).astype(np.float32)
            blk[5] = -amax
            x = (blk * np.float32(2.0 ** s)).astype(np.float32)
            _, scales = S.quantize_sr(x, fmt, np.zeros(32, dtype=np.uint32))
            _, near = Q.quantize(x, fmt)
            assert int(scales[0]) == int(near[0]) + int(bumped), (s, amax)
            assert int(near[0]) == s + 127
    # all-zero block: byte 0; non-finite: 255 and code 0; clamp to byte 0 at the bottom
    z = np.zeros(96, dtype=np.float32)
    z[32:64] = -0.0
    z[64:] = 2.0 ** -140
    codes, scales = S.quantize_sr(z, fmt, np.zeros(96, dtype=np.uint32))
    assert list(scales) == [0, 0, 0] and (codes[:32] == 0).all() and (codes[32:64] == 1 << (Q.FORMATS[fmt]["bits"] - 1)).all()
    bad = np.ones(64, dtype=np.float32)
    bad[3], bad[40] = np.nan, np.inf
    codes, scales = S.quantize_sr(bad, fmt, np.zeros(64, dtype=np.uint32))
    assert list(scales) == [255, 255] and not codes.any()


@pytest.mark.parametrize("fmt", FMTS)
def test_the_reference_is_unbiased_on_the_gpu_tests_inputs(fmt):
    """tests/test_gpu_sr.py's unbiasedness case on the reference alone: the mean of D(Q(x)) over
    steps 0..255 lies within 0.2 grid steps of x for every element (Hoeffding: each error lies inside
    one grid step, so P(any of 4096 elements leaves +-0.2) <= 4096 * 2 exp(-2 * 256 * 0.04) ~ 1e-5),
    while nearest rounding — whose mean is its one error — misses it for at least a quarter."""
    x = S.unbiased_inputs()
    acc = np.zeros(x.size)
    for step in range(256):
        codes, scales = S.sr_quantize(x, fmt, S.UNBIASED_SEED, step, 0)
        d = Q.dequantize(codes, scales, fmt)
        assert (np.abs(d - x) < S.grid_step(x, fmt)).all()
        acc += d
    worst = (np.abs(acc / 256 - x) / S.grid_step(x, fmt)).max()
    print("max |mean - x| / grid step:", fmt, worst)
    assert worst <= 0.2
    codes, scales = Q.quantize(x, fmt)
    miss = np.abs(Q.dequantize(codes, scales, fmt) - x) / S.grid_step(x, fmt, scales) > 0.2
    print("nearest: fraction outside 0.2 steps:", fmt, miss.mean())
    assert miss.mean() >= 0.25


# ---------------------------------------------------------------------------------------------
# host-side validation of the C ABI (no GPU: every call fails before any HIP call)

@pytest.fixture(scope="module")
def lib():
    if torch.cuda.is_available():
        pytest.skip("host-pointer validation: CPU-only (a device run would launch on host addresses)")
    from evolutionarydistributedtraining_amd import _lib
    return _lib.load_library()


_host = (ctypes.c_uint8 * 4096)()
_P = ctypes.c_void_p


def _fake(i, skew=0):
    return _P(ctypes.addressof(_host) // 64 * 64 + 64 * (i + 1) + skew)     # never dereferenced


def test_abi_validation_of_the_stochastic_entries(lib):
    def err():
        return lib.edt_last_error().decode()

    ws = (_P * 2)(_fake(1), _fake(2))
    ws_odd = (_P * 2)(_fake(1), _fake(2, 8))
    ws_null = (_P * 2)(_fake(1), None)

    def part(n=1024, region=512, fmt=0, gdt=0, wdt=1, k=2, kt=2, theta=_fake(0), workers=ws, packed=_fake(3), base=0):
        return lib.edt_delta_partial_q_sr(theta, gdt, workers, wdt, k, kt, n, region, fmt, packed, 7, 1, 0, base, None)

    assert part(fmt=2) < 0 and "wire format" in err()
    assert part(fmt=-1) < 0 and "wire format" in err()
    assert part(n=1536, region=1024) < 0 and "whole number of regions" in err()
    assert part(region=500) < 0 and "multiple of 512" in err()
    assert part(region=0) < 0 and "multiple of 512" in err()
    for base in (4, 1, 1025):
        assert part(base=base) < 0 and "elem_base" in err() and "multiple of 8" in err()
    assert part(gdt=1, wdt=0) < 0 and "dtype" in err()
    assert part(k=0) < 0 and "worker count" in err()
    assert part(k=65) < 0 and "worker count" in err()
    assert part(kt=0) < 0 and "total worker count" in err()
    assert part(theta=None) < 0 and "theta_g is null" in err()
    assert part(workers=None) < 0 and "theta_k is null" in err()
    assert part(workers=ws_null) < 0 and "theta_k[1] is null" in err()
    assert part(packed=None) < 0 and "packed is null" in err()
    for kw in ({"theta": _fake(0, 8)}, {"workers": ws_odd}, {"packed": _fake(3, 4)}):
        assert part(**kw) < 0 and "16-byte aligned" in err(), kw
    assert part(n=0) == 0 and part(n=0, base=1 << 40) == 0            # nothing to do, nothing launched

    regs = (_P * 2)(_fake(1), _fake(2))
    odd = (_P * 2)(_fake(1), _fake(2, 8))
    null = (_P * 2)(_fake(1), None)

    def delta(n=512, fin=0, fout=0, nacc=2, gdt=0, theta=_fake(0), regions=regs, mom=_fake(3), out=_fake(5), mu=0.9,
              base=0):
        return lib.edt_sgd_delta_sum_q_sr(theta, gdt, regions, nacc, fin, mom, 1, n, 0.7, mu, 1, out, fout, 7, 1, 1,
                                          base, None)

    assert delta(fin=2) < 0 and "wire format" in err()
    assert delta(fout=-1) < 0 and "wire format" in err()
    assert delta(fin=1, fout=7) < 0 and "wire format 7" in err()
    assert delta(nacc=0) < 0 and "partial count" in err()
    assert delta(nacc=65) < 0 and "partial count" in err()
    assert delta(n=500) < 0 and "multiple of 512" in err()
    for base in (4, 513):
        assert delta(base=base) < 0 and "elem_base" in err() and "multiple of 8" in err()
    assert delta(gdt=3) < 0 and "dtype" in err()
    assert delta(theta=None) < 0 and "null" in err()
    assert delta(regions=None) < 0 and "null" in err()
    assert delta(regions=null) < 0 and "regions[1] is null" in err()
    assert delta(out=None) < 0 and "packed_out is null" in err()
    assert delta(mom=None) < 0 and "momentum buffer is null" in err()
    for kw in ({"theta": _fake(0, 8)}, {"regions": odd}, {"mom": _fake(3, 4)}, {"out": _fake(5, 8)}):
        assert delta(**kw) < 0 and "16-byte aligned" in err(), kw
    assert delta(n=0) == 0
    assert lib.edt_abi_version() == 6                                  # two entries added, no revision


# ---------------------------------------------------------------------------------------------
# ShardedOuterSync: options, then the schedule through the kernels= seam on CPU tensors

def _make(world=2, **kw):
    from evolutionarydistributedtraining_amd.collectives import VirtualWorld
    from evolutionarydistributedtraining_amd.distributed import ShardedOuterSync
    from evolutionarydistributedtraining_amd.params import ParamLayout
    kw.setdefault("kernels", object())
    return ShardedOuterSync(ParamLayout([(1000,)]), torch.float32, torch.bfloat16, 4, "cpu",
                            comm=VirtualWorld(world).comm(0), **kw)


def test_option_handling():
    with pytest.raises(ValueError, match="error_feedback"):
        _make(mode="reduce_q", rounding="stochastic", error_feedback=True)
    with pytest.raises(ValueError, match="error_feedback"):
        _make(mode="reduce_q", rounding="stochastic")                         # error feedback is the default
    for mode in ("reduce", "reduce_ordered", "exact", "auto"):
        with pytest.raises(ValueError, match="reduce_q"):
            _make(mode=mode, rounding="stochastic", error_feedback=False)
    with pytest.raises(ValueError, match="rounding"):
        _make(mode="reduce_q", rounding="up", error_feedback=False)
    with pytest.raises(ValueError, match="seed"):
        _make(mode="reduce_q", rounding="stochastic", error_feedback=False, seed=-1)
    for gf in (None, "mxfp8", "mxfp4"):
        s = _make(mode="reduce_q", rounding="stochastic", error_feedback=False, gather_format=gf, seed=11)
        off = _make(mode="reduce_q", error_feedback=False, gather_format=gf)
        on = _make(mode="reduce_q", error_feedback=True, gather_format=gf)
        assert s.residual is None and (gf is None or s.residual_g is None)     # no residual buffers
        assert (s.rounding, s.seed, s.q_step, off.rounding, off.q_step) == ("stochastic", 11, 0, "nearest", 0)
        assert s.wire_bytes() == off.wire_bytes()
        # kernel_bytes(): the error-feedback-off count, from distributed.py's formula (n_pad = 1024,
        # world 2, K_local 4 bf16 workers, fp32 theta, momentum)
        n_pad, shard, wb, gb = 1024, 512, 2, 4
        q = lambda elems, f="mxfp8": elems * Q.FORMATS[f]["bits"] // 8 + elems // 32
        p1 = n_pad * (4 * wb + gb) + q(n_pad)
        if gf is None:
            want = p1 + shard * (2 * gb + 2 * gb) + 2 * q(shard)
        else:
            want = p1 + shard * (gb + 2 * gb) + 2 * q(shard) + q(shard, gf) + n_pad * 2 * gb + q(n_pad, gf)
        assert s.kernel_bytes() == off.kernel_bytes() == want
        assert on.kernel_bytes() == want + 8 * n_pad + (8 * shard if gf else 0)


class _Recorder:
    """Stand-in kernels that record the keywords the schedule passes."""

    def __init__(self):
        self.calls = []

    def delta_partial_q(self, theta, workers, k_total, packed, region_elems, fmt, residual=None, **kw):
        self.calls.append(("p1", theta.numel(), region_elems, residual, kw))

    def sgd_apply_sum_q(self, *a):
        self.calls.append(("p2", a[0].numel()))

    def sgd_delta_sum_q(self, theta, regions, fmt_in, mom, has, lr, mu, nesterov, packed_out, fmt_out, residual=None, **kw):
        self.calls.append(("p2'", theta.numel(), fmt_out, residual, kw))

    def apply_delta_q(self, *a):
        self.calls.append(("p3",))


def test_q_step_advances_and_the_keywords_reach_the_kernels():
    from evolutionarydistributedtraining_amd.collectives import VirtualWorld
    from evolutionarydistributedtraining_amd.distributed import ShardedOuterSync
    from evolutionarydistributedtraining_amd.params import ParamLayout
    layout = ParamLayout([(3000,)])

    def body(comm):
        rec = _Recorder()
        s = ShardedOuterSync(layout, torch.float32, torch.bfloat16, 2, "cpu", mode="reduce_q", error_feedback=False,
                             rounding="stochastic", seed=99, gather_format="mxfp4", bucket_elems=2048, kernels=rec,
                             comm=comm)
        assert s.buckets == [(0, 2048), (2048, 3072)] and s.q_step == 0
        s.step()
        s.step()
        assert s.q_step == 2
        s.q_step = 40                                                 # settable: a restart restores it
        s.step()
        assert s.q_step == 41
        return rec, s.buckets

    for rank, (rec, buckets) in enumerate(VirtualWorld(2).run(body)):
        p1 = [c for c in rec.calls if c[0] == "p1"]
        p2 = [c for c in rec.calls if c[0] == "p2'"]
        assert len(p1) == len(p2) == 6 and not [c for c in rec.calls if c[0] == "p2"]
        want_steps = [0, 0, 1, 1, 40, 40]
        for i, (c, d) in enumerate(zip(p1, p2)):
            b, e = buckets[i % 2]
            per = (e - b) // 2
            assert c[3] is None and d[3] is None
            assert c[4] == {"rounding": "stochastic", "seed": 99, "step": want_steps[i], "stream_id": 2 * rank,
                            "elem_base": b}
            assert d[4] == {"rounding": "stochastic", "seed": 99, "step": want_steps[i], "stream_id": 2 * rank + 1,
                            "elem_base": b + rank * per}
    # nearest mode passes no new keyword (stand-in kernels without them keep working) and counts steps too
    def plain(comm):
        rec = _Recorder()
        s = ShardedOuterSync(layout, torch.float32, torch.bfloat16, 2, "cpu", mode="reduce_q", error_feedback=False,
                             gather_format="mxfp8", bucket_elems=2048, kernels=rec, comm=comm)
        s.step()
        return rec, s.q_step

    for rec, q_step in VirtualWorld(2).run(plain):
        assert q_step == 1 and len(rec.calls) == 6 and all(c[4] == {} for c in rec.calls if c[0] in ("p1", "p2'"))


SHAPES = [(37, 11), (5,), (1,), (64, 33), (129,), (300,), (7, 401)]


def _run(*a, **kw):
    return S.run_schedule(*a, **kw)


def _oracle_fns(oracle):
    def partial(th, pads, K):
        acc = torch.zeros(th.numel(), dtype=torch.float32)
        oracle.delta_partial(th, pads, K, acc, False)
        return acc.numpy()

    def sgd_sum(new, ds, mom, has, lr, mu, nesterov):
        total = ds[0].clone()
        for d in ds[1:]:
            total.add_(d)
        oracle.sgd_apply(new, total, mom, has, lr, mu, nesterov)

    return partial, sgd_sum


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("fmt_in,fmt_out", [("mxfp8", None), ("mxfp4", None), ("mxfp8", "mxfp8"), ("mxfp4", "mxfp8"),
                                            ("mxfp8", "mxfp4")])
@pytest.mark.parametrize("tdt,wdt", [(torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16)])
def test_stochastic_schedule_through_the_kernels_seam(oracle, world, fmt_in, fmt_out, tdt, wdt):
    layout, theta, gens = population(SHAPES, tdt, wdt, 4, steps=3)
    seed = 0x1234567890abcdef
    res = _run(world, layout, tdt, wdt, theta, gens, S.NumpySrKernels(oracle), fmt_in, fmt_out, seed, world * 512)
    n_pad, buckets = res[0]["n_pad"], res[0]["buckets"]
    assert len(buckets) >= 2 and n_pad > layout.total and res[0]["q_step"] == 3 and not res[0]["has_residual"]
    for r in res:
        for a, b in zip(r["steps"], res[0]["steps"]):
            assert torch.equal(bits(a["theta"]), bits(b["theta"]))
    th, mom = S.compose(*_oracle_fns(oracle), theta, gens, world, n_pad, buckets, fmt_in, fmt_out, seed)
    assert torch.equal(bits(res[0]["steps"][-1]["theta"]), bits(th))
    own = S.owners(buckets, world, n_pad)
    for r in range(world):
        assert torch.equal(bits(res[r]["steps"][-1]["mom"]), bits(mom[torch.from_numpy(np.flatnonzero(own == r))])), r
    # it is not the nearest schedule, and another seed draws other bits
    near = _run(world, layout, tdt, wdt, theta, gens, S.NumpySrKernels(oracle), fmt_in, fmt_out, seed, world * 512,
                rounding="nearest")
    assert not torch.equal(bits(near[0]["steps"][-1]["theta"]), bits(th))
    other = _run(world, layout, tdt, wdt, theta, gens[:1], S.NumpySrKernels(oracle), fmt_in, fmt_out, seed + 1, world * 512)
    assert not torch.equal(bits(other[0]["steps"][0]["theta"]), bits(res[0]["steps"][0]["theta"]))


def test_nearest_mode_still_takes_kernels_without_the_keywords(oracle):
    layout, theta, gens = population(SHAPES, torch.float32, torch.bfloat16, 4, steps=2)
    a = _run(2, layout, torch.float32, torch.bfloat16, theta, gens, G.NumpyGatherKernels(oracle), "mxfp8", "mxfp8", 0,
             1024, rounding="nearest")
    b = _run(2, layout, torch.float32, torch.bfloat16, theta, gens, S.NumpySrKernels(oracle), "mxfp8", "mxfp8", 5,
             1024, rounding="nearest")
    assert torch.equal(bits(a[0]["steps"][-1]["theta"]), bits(b[0]["steps"][-1]["theta"]))


def test_a_restart_that_restores_q_step_replays_the_same_bits(oracle):
    tdt, wdt = torch.float32, torch.bfloat16
    layout, theta, gens = population(SHAPES, tdt, wdt, 4, steps=3)
    k = S.NumpySrKernels(oracle)
    full = _run(2, layout, tdt, wdt, theta, gens, k, "mxfp8", "mxfp4", 77, 1024)
    state = [r["steps"][0] for r in full]
    again = _run(2, layout, tdt, wdt, theta, gens[1:], k, "mxfp8", "mxfp4", 77, 1024, first_step=1, state=state)
    for r in range(2):
        for a, b in zip(again[r]["steps"], full[r]["steps"][1:]):
            assert torch.equal(bits(a["theta"]), bits(b["theta"])) and torch.equal(bits(a["mom"]), bits(b["mom"]))
    wrong = _run(2, layout, tdt, wdt, theta, gens[1:], k, "mxfp8", "mxfp4", 77, 1024, first_step=0, state=state)
    assert not torch.equal(bits(wrong[0]["steps"][0]["theta"]), bits(full[0]["steps"][1]["theta"]))


def test_the_wrappers_refuse_a_residual_before_any_device_work():
    from evolutionarydistributedtraining_amd import ops
    assert ops.ROUNDING == {"nearest": 0, "stochastic": 1}
    with pytest.raises(ops.L.EdtError, match="residual"):
        ops._stochastic("stochastic", torch.zeros(8), 0, 0, 0, 0)
    with pytest.raises(ops.L.EdtError, match="elem_base"):
        ops._stochastic("stochastic", None, 0, 0, 0, 4)
    with pytest.raises(ops.L.EdtError, match="rounding"):
        ops._stochastic("even", None, 0, 0, 0, 0)
    assert ops._stochastic("stochastic", None, (1 << 64) - 1, 5, 3, 1 << 33) and not ops._stochastic("nearest", None, 0, 0, 0, 0)
