"""The fp32 fused step's residency cap (EDT_OUTER_WG_PER_CU, edt_common.h) changes where workgroups
run, never what they compute (needs an MI355X).

The library is built three times into a temporary directory: as committed (the default cap), with
-DEDT_OUTER_WG_PER_CU=1 (one workgroup per CU: the largest dynamic-LDS request a launch can make,
160 KB, whatever the default becomes) and with -DEDT_OUTER_WG_PER_CU=0 (uncapped, no LDS request).
Three steps with a carried momentum buffer and Nesterov on, same fixed-seed inputs: theta and the
momentum of either capped build must agree with the uncapped build's bit for bit after every step,
and every call must return success. No tolerances. The cap applies at K = 8 (the measured mix);
K = 3 launches uncapped in every build and must agree all the same.
"""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import pytest
import torch

pytestmark = pytest.mark.gpu

TILE = 2048                       # 256 threads x 8 elements
# several tiles + a scalar tail longer than one wave; the tail alone; exactly one tile, no tail
SIZES = [TILE * 5 + 1037, 1037, TILE]
WORKERS = [8, 3]                  # K = 8: multiply by 1/K; K = 3: true division
STEPS = 3
LR, MU = 0.7, 0.9


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def libs(dev, tmp_path_factory):
    """{name: bound library} for the default, cap-1 and uncapped builds (built only where a device is)."""
    from evolutionarydistributedtraining_amd import _lib, build
    d = tmp_path_factory.mktemp("window")
    jobs = [("default", None), ("cap1", ["-DEDT_OUTER_WG_PER_CU=1"]), ("uncapped", ["-DEDT_OUTER_WG_PER_CU=0"])]
    with ThreadPoolExecutor(max_workers=len(jobs)) as pool:
        paths = list(pool.map(lambda j: build.build_library(force=True, out=str(d / f"libedt_{j[0]}.so"), extra_flags=j[1]),
                              jobs))
    return {j[0]: _lib.load_library(p) for j, p in zip(jobs, paths)}


def run_steps(lib, dev, n, k):
    """theta and momentum after each of STEPS carried-momentum steps, as int32 bit patterns."""
    from evolutionarydistributedtraining_amd import _lib
    g = torch.Generator(device="cpu").manual_seed(1234 + 7 * k + n % 1000)
    theta = torch.randn(n, generator=g).to(dev)
    mom = (0.01 * torch.randn(n, generator=g)).to(dev)
    workers = [(theta.cpu() + 0.05 * torch.randn(n, generator=g)).to(dev) for _ in range(k)]
    out = []
    for _ in range(STEPS):
        rc = lib.edt_outer_step(_lib.ptr(theta), _lib.EDT_F32, _lib.ptr_array(workers), _lib.EDT_F32, k, _lib.ptr(mom), 1,
                                ctypes.c_uint64(n), LR, MU, 1, _lib.stream_ptr(dev))
        assert rc == 0, lib.edt_last_error().decode(errors="replace")
        torch.cuda.synchronize(dev)
        out.append((theta.view(torch.int32).clone(), mom.view(torch.int32).clone()))
    return out


@pytest.fixture(scope="module")
def uncapped_steps(libs, dev):
    """The uncapped build's results, computed once per (n, K)."""
    return {(n, k): run_steps(libs["uncapped"], dev, n, k) for n in SIZES for k in WORKERS}


@pytest.mark.parametrize("build_name", ["default", "cap1"])
@pytest.mark.parametrize("k", WORKERS)
@pytest.mark.parametrize("n", SIZES)
def test_cap_is_bit_identical_to_uncapped(libs, uncapped_steps, dev, n, k, build_name):
    capped, uncapped = run_steps(libs[build_name], dev, n, k), uncapped_steps[(n, k)]
    for step, ((t0, m0), (t1, m1)) in enumerate(zip(capped, uncapped)):
        assert torch.equal(t0, t1), f"theta differs after step {step + 1} (n = {n}, K = {k})"
        assert torch.equal(m0, m1), f"momentum differs after step {step + 1} (n = {n}, K = {k})"
    assert not torch.equal(capped[0][0], capped[-1][0])          # the steps did move theta
