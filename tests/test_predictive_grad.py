"""CPU tier of kvae_lgssm_predictive_bwd / lgssm_ops.PredictiveLogLik / KalmanFilter.log_marginal / the "marginal" objective: the
host simulation injected (as tests/test_predictive.py does), so the adjoint launch runs the kernel bodies of csrc/lgssm_pred.h on
emulated wavefronts (tests/hostsim/wave_emu.h) and the model level runs on the host simulation.  The cases are
tests/pred_grad_cases.py (the GPU tier runs the same ones); here also: which body ran for each shape (the emulator's launch
counters), the yardstick constants, the resource report of the gfx950 kernels, and the bodies under ASan + UBSan."""
import os
import re
import subprocess
from pathlib import Path

import pytest
import torch

import pred_grad_cases as cases
from hostsim.build import build as build_hostsim

torch.set_num_threads(4)
ROOT = Path(__file__).resolve().parents[1]
N4, N16, RT = 0, 1, 2   # kvae_wemu_predictive_bwd_launches(which)


@pytest.fixture(scope="module", autouse=True)
def wave_emu_backend():
    from kvae import _native
    lib = _native.LgssmLib(build_hostsim())
    _native._set_test_backend(lib)
    lib.dll.kvae_hostsim_wave_emu(1)
    yield lib
    lib.dll.kvae_hostsim_wave_emu(0)
    _native._set_test_backend(None)


def launches(lib):
    return [lib.dll.kvae_wemu_predictive_bwd_launches(k) for k in range(3)]   # csrc/lgssm_pred.h, KVAE_WAVE_EMU section


def body_of(n):
    return N4 if n == 4 else (N16 if n == 16 else RT)


def test_yardsticks_are_what_float32_torch_gives():
    """The constants the bars derive from: float32 autograd of log_marginal_torch against float64, remeasured.  Each is the largest
    of a few thousand rounding samples and moves with the host's vector width and libm: within a factor 3 either way."""
    got = cases.yardsticks()
    print({k: float(f"{v:.3g}") for k, v in got.items()})
    for k, v in got.items():
        assert v / 3 <= cases.YARDSTICK[k] <= v * 3, (k, v, cases.YARDSTICK[k])


_WORST = {}


@pytest.mark.parametrize("cmode,masked", [("shared", True), ("packed", True), ("shared", False), ("packed", False)])
@pytest.mark.parametrize("B,T,n", cases.SHAPES)
def test_per_item_vs_float64(wave_emu_backend, B, T, n, cmode, masked):
    before = launches(wave_emu_backend)
    cases.check(wave_emu_backend, "cpu", B, T, n, cmode, masked, worst=_WORST)
    want = [0, 0, 0]
    want[body_of(n)] = 1                                                   # the body built for this n is what ran, once
    assert [a - b for a, b in zip(launches(wave_emu_backend), before)] == want
    print("worst so far", {k: float(f"{v:.3g}") for k, v in _WORST.items()})


@pytest.mark.parametrize("B,T,n", [(3, 37, 4), (5, 13, 16)])
def test_unaligned_operands_take_the_runtime_body(wave_emu_backend, B, T, n):
    """Every operand and output a view offset by one float, and C_t / gC in a record whose slot is not 16-byte aligned: the
    4-byte-access body, same bars."""
    before = launches(wave_emu_backend)
    cases.check(wave_emu_backend, "cpu", B, T, n, "shared", True, unaligned=True)
    cases.check(wave_emu_backend, "cpu", B, T, n, "packed", True, pad=3)
    assert [a - b for a, b in zip(launches(wave_emu_backend), before)] == [0, 0, 2]


@pytest.mark.parametrize("B,T,n", [(3, 5, 4), (2, 3, 16), (3, 5, 7)])
def test_upstream_variants(wave_emu_backend, B, T, n):
    cases.upstream_variants(wave_emu_backend, "cpu", B, T, n)


@pytest.mark.parametrize("B,T,n", [(3, 5, 4), (2, 3, 16), (3, 5, 7)])
def test_partial_outputs_and_repeatability(wave_emu_backend, B, T, n):
    cases.partial_outputs(wave_emu_backend, "cpu", B, T, n)


@pytest.mark.parametrize("cmode", cases.CMODES)
@pytest.mark.parametrize("B,T,n", [(3, 5, 4), (2, 3, 16), (3, 5, 7)])
def test_autograd_function(wave_emu_backend, B, T, n, cmode):
    before = launches(wave_emu_backend)
    cases.function_matches_raw(wave_emu_backend, "cpu", B, T, n, cmode)
    assert launches(wave_emu_backend)[body_of(n)] >= before[body_of(n)] + 2


@pytest.mark.parametrize("n", [4, 16, 5])
def test_ladder_levels_3_and_5(wave_emu_backend, n):
    before = launches(wave_emu_backend)
    cases.ladder(wave_emu_backend, "cpu", n)
    assert launches(wave_emu_backend)[body_of(n)] == before[body_of(n)] + 1


@pytest.mark.parametrize("B,T,n", [(2, 5, 4), (2, 4, 16)])
def test_joint_gaussian_gradient(wave_emu_backend, B, T, n):
    before = launches(wave_emu_backend)
    cases.joint_gaussian_grad("cpu", B, T, n)
    assert launches(wave_emu_backend)[body_of(n)] == before[body_of(n)] + 1


def test_c_entry_point_rejects(wave_emu_backend):
    cases.c_abi(wave_emu_backend, "cpu")


def test_unsupported_shapes_take_torch(wave_emu_backend):
    cases.unsupported_takes_torch("cpu")


def test_torch_fallback_has_the_forward_values_and_finite_gradients():
    cases.torch_values_are_predictive_torch()


def test_host_tensors_take_torch_without_a_backend():
    """Product behaviour on host tensors (no test backend): log_marginal falls back to torch, forcing the kernel raises."""
    from kvae import _native
    from kvae.kalman import lgssm_ops
    saved = _native._test_backend
    _native._set_test_backend(None)
    try:
        k = cases.pc.inputs(2, 5, 4, "shared")["k"]
        Y = k["Y"].clone().requires_grad_(True)
        lgssm_ops.log_marginal(k["mp"], k["Sp"], k["C"], k["R"], Y, k["mask"])["seq_ll"].sum().backward()
        assert bool(torch.isfinite(Y.grad).all()) and bool(Y.grad.any())
        with pytest.raises(RuntimeError):
            lgssm_ops.log_marginal(k["mp"], k["Sp"], k["C"], k["R"], k["Y"], k["mask"], impl="kernel")
    finally:
        _native._set_test_backend(saved)


# ---- model level ------------------------------------------------------------------------------------------------------------
def test_model_yardsticks_are_what_float32_torch_gives(wave_emu_backend):
    got = cases.model_yardsticks()
    print({k: float(f"{v:.3g}") for k, v in got.items()})
    for k, v in got.items():
        assert v / 3 <= cases.MODEL_YARDSTICK[k] <= v * 3, (k, v, cases.MODEL_YARDSTICK[k])


@pytest.mark.parametrize("kind,K", cases.MODELS)
def test_kalman_filter_log_marginal(wave_emu_backend, kind, K):
    before = launches(wave_emu_backend)
    cases.model_log_marginal("cpu", kind, K)
    assert launches(wave_emu_backend)[N4] == before[N4] + 1


@pytest.mark.parametrize("kind,K", cases.MODELS)
def test_compute_loss_marginal(wave_emu_backend, kind, K):
    before = launches(wave_emu_backend)
    cases.model_compute_loss("cpu", kind, K)
    assert launches(wave_emu_backend)[N4] == before[N4] + 1   # the one "marginal" step; the two "elbo" steps launch none


def test_errors(wave_emu_backend):
    cases.model_errors("cpu")


# ---- the gfx950 build and the sanitizers --------------------------------------------------------------------------------------
def test_kernels_have_no_scratch():
    """The resource report of the adjoint kernels (gfx950 cross-compile): 0 bytes of scratch per lane."""
    src = ROOT / "kalman-vae_amd" / "csrc" / "kvae_lgssm_pred_bwd.hip"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-amdgpu-mfma-vgpr-form", "-c",
                        str(src), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S*k_pred_bwd_\S*)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == 3 and len(scratch) == 3, (names, scratch)
    assert all(s == 0 for s in scratch), list(zip(names, scratch))


def test_kernel_bodies_under_sanitizers():
    """A standalone driver of the adjoint bodies on emulated wavefronts (tests/hostsim/pred_bwd_asan_driver.cpp), built with
    -fsanitize=address,undefined and run as a child process: all three bodies, ragged B*T, gC in a packed record, every buffer at
    its exact size."""
    out = ROOT / "tests" / "hostsim" / "pred_bwd_asan_driver"
    src = ROOT / "tests" / "hostsim" / "pred_bwd_asan_driver.cpp"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-fno-sanitize-recover=undefined", "-o", str(out), str(src)], check=True, cwd=ROOT)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(out)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "PRED-BWD-ASAN-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
