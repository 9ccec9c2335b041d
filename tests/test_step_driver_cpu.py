"""ShardedOuterSync.step(): the order of local launches and collective calls of every schedule,
on rank 0 of 2 with two buckets, recording stand-ins for the kernels and the communicator (no GPU,
nothing is computed). The expected sequences are written out by hand: per bucket, the produce side
(local launch, then its collective) of every bucket comes before the first wait; then per bucket
the wait, the step on the owned shard and its gather; the quantized gather's phase 3 runs after all
of phase 2'; the gathers are waited for last."""
import pytest
import torch

from evolutionarydistributedtraining_amd.collectives import Collectives
from evolutionarydistributedtraining_amd.distributed import ShardedOuterSync
from evolutionarydistributedtraining_amd.params import ParamLayout

WORLD, K_LOCAL, BUCKET = 2, 2, 1024


def _bucket(t: torch.Tensor) -> int:
    """Which of the two equal buckets a slice of a per-step buffer starts in."""
    base = t._base if t._base is not None else t
    return int(2 * t.storage_offset() >= base.numel())


class _Handle:
    def __init__(self, log, what, bucket):
        self.log, self.what, self.bucket = log, what, bucket

    def wait(self):
        self.log.append(("wait " + self.what, self.bucket))


class _Comm(Collectives):
    inplace = True

    def __init__(self, log):
        self.world, self.rank, self.log = WORLD, 0, log

    def _call(self, what, t):
        self.log.append((what, _bucket(t)))
        return _Handle(self.log, what, _bucket(t))

    def reduce_scatter(self, out, inp, async_op=False):
        return self._call("reduce_scatter", inp)

    def all_to_all(self, out, inp, async_op=False):
        return self._call("all_to_all", inp)

    def all_gather(self, out, inp, async_op=False):
        return self._call("all_gather", out)


class _Kernels:
    """Every local kernel records (its name, the bucket of its theta slice) and the element offset of
    the momentum slice it was handed."""
    NAMES = ("delta_partial", "sgd_apply", "sgd_apply_sum", "delta_partial_q", "sgd_apply_sum_q", "sgd_delta_sum_q",
             "apply_delta_q", "outer_step")

    def __init__(self, log, moms):
        for name in self.NAMES:
            setattr(self, name, self._recorder(name, log, moms))

    @staticmethod
    def _recorder(name, log, moms):
        def call(theta, *args, **kw):
            log.append((name, _bucket(theta)))
            for a in args:
                if torch.is_tensor(a) and a._base is not None and a._base.numel() == BUCKET and a.dtype == theta.dtype:
                    moms.append((name, a.storage_offset(), a.numel()))
        return call


def _steps(mode, **kw):
    log, moms = [], []
    s = ShardedOuterSync(ParamLayout([(2 * BUCKET,)]), torch.float32, torch.bfloat16, K_LOCAL, "cpu", mode=mode,
                         broadcast="theta", bucket_elems=BUCKET, kernels=_Kernels(log, moms), comm=_Comm(log), **kw)
    assert s.buckets == [(0, BUCKET), (BUCKET, 2 * BUCKET)] and s.mom_shard.numel() == BUCKET
    s.step()
    return s, log, moms


def _produce_then_consume(produce, collective, step, extra=()):
    """The hand-written shape of a two-bucket step with one collective per bucket."""
    return ([(produce, 0), (collective, 0), (produce, 1), (collective, 1)] if produce else []) + [
        ("wait " + collective, 0), (step, 0), ("all_gather", 0),
        ("wait " + collective, 1), (step, 1), ("all_gather", 1),
        *extra, ("wait all_gather", 0), ("wait all_gather", 1)]


def test_reduce_order():
    s, log, moms = _steps("reduce")
    assert log == _produce_then_consume("delta_partial", "reduce_scatter", "sgd_apply")
    assert moms == [("sgd_apply", 0, 512), ("sgd_apply", 512, 512)]
    assert s.has_momentum and s.q_step == 1


def test_reduce_ordered_order():
    _, log, moms = _steps("reduce_ordered")
    assert log == _produce_then_consume("delta_partial", "all_to_all", "sgd_apply_sum")
    assert moms == [("sgd_apply_sum", 0, 512), ("sgd_apply_sum", 512, 512)]


def test_reduce_q_order():
    _, log, moms = _steps("reduce_q")
    assert log == _produce_then_consume("delta_partial_q", "all_to_all", "sgd_apply_sum_q")
    assert moms == [("sgd_apply_sum_q", 0, 512), ("sgd_apply_sum_q", 512, 512)]


def test_reduce_q_gather_format_order():
    """Phase 3 (apply_delta_q as each bucket's updates land) starts after all of phase 2'."""
    _, log, moms = _steps("reduce_q", gather_format="mxfp8")
    phase3 = [("wait all_gather", 0), ("apply_delta_q", 0), ("wait all_gather", 1), ("apply_delta_q", 1)]
    assert log == _produce_then_consume("delta_partial_q", "all_to_all", "sgd_delta_sum_q", phase3)
    # the momentum slice and the owner's residual slice (same dtype, same offsets) of each bucket
    assert moms == [("sgd_delta_sum_q", 0, 512)] * 2 + [("sgd_delta_sum_q", 512, 512)] * 2


def test_exact_order():
    """One all-to-all per local worker and bucket, all issued first; a bucket's are all waited for
    before its fused step."""
    _, log, moms = _steps("exact")
    assert log == [("all_to_all", 0)] * 2 + [("all_to_all", 1)] * 2 + [
        ("wait all_to_all", 0), ("wait all_to_all", 0), ("outer_step", 0), ("all_gather", 0),
        ("wait all_to_all", 1), ("wait all_to_all", 1), ("outer_step", 1), ("all_gather", 1),
        ("wait all_gather", 0), ("wait all_gather", 1)]
    assert moms == [("outer_step", 0, 512), ("outer_step", 512, 512)]


@pytest.mark.parametrize("mode", ["reduce", "reduce_q"])
def test_kernel_events_bracket_every_local_launch(mode):
    """kernel_events: one (start, end) pair per local kernel, in launch order."""
    log, moms, made = [], [], []

    class Ev:
        def __init__(self):
            made.append(self)

        def record(self):
            log.append(("event", made.index(self)))

    s = ShardedOuterSync(ParamLayout([(2 * BUCKET,)]), torch.float32, torch.bfloat16, K_LOCAL, "cpu", mode=mode,
                         broadcast="theta", bucket_elems=BUCKET, kernels=_Kernels(log, moms), comm=_Comm(log))
    s.event_factory = Ev
    s.kernel_events = []
    s.step()
    assert len(s.kernel_events) == 4 and [made.index(a) for a, _ in s.kernel_events] == [0, 2, 4, 6]
    kernels = [i for i, (name, _) in enumerate(log) if name in _Kernels.NAMES]
    assert len(kernels) == 4
    for i in kernels:
        assert log[i - 1][0] == "event" and log[i + 1][0] == "event"
