"""CPU tier of kvae_lgssm_predictive / KalmanFilter.predictive / KVAE.score / KVAE.log_likelihood: the host simulation injected
(as tests/test_posterior_sample.py does), so the item and sequence launches run the kernel bodies of csrc/lgssm_pred.h on
emulated wavefronts (tests/hostsim/wave_emu.h) and the model level runs on the host simulation.  The cases are
tests/pred_cases.py (the GPU tier runs the same ones); here also: which body ran for each shape (the emulator's launch counters),
the yardstick constants, the resource report of the gfx950 kernels, and the bodies under ASan + UBSan."""
import itertools
import os
import re
import subprocess
from pathlib import Path

import pytest
import torch

import pred_cases as cases
from hostsim.build import build as build_hostsim

torch.set_num_threads(4)
ROOT = Path(__file__).resolve().parents[1]
N4, N16, RT, SEQ = 0, 1, 2, 3   # kvae_wemu_predictive_launches(which)


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
    return [lib.dll.kvae_wemu_predictive_launches(k) for k in range(4)]   # csrc/lgssm_pred.h, KVAE_WAVE_EMU section


def body_of(n):
    return N4 if n == 4 else (N16 if n == 16 else RT)


def test_yardsticks_are_what_float32_torch_gives():
    """The constants the bars derive from: the float32 restatement against the float64 one, remeasured.  Each is the largest
    of a few thousand rounding samples and moves with the host's vector width and libm: within a factor 3 either way."""
    for k, v in cases.yardsticks().items():
        assert v / 3 <= cases.YARDSTICK[k] <= v * 3, (k, v, cases.YARDSTICK[k])


@pytest.mark.parametrize("cmode,masked", [("shared", True), ("packed", True), ("shared", False)])
@pytest.mark.parametrize("B,T,n", cases.SHAPES + cases.SEQ_SHAPES)
def test_per_item_vs_float64(wave_emu_backend, B, T, n, cmode, masked):
    before = launches(wave_emu_backend)
    cases.check("cpu", B, T, n, cmode, masked)
    after = launches(wave_emu_backend)
    want = [0, 0, 0, 1]
    want[body_of(n)] = 1                                                   # the body built for this n is what ran, once
    assert [a - b for a, b in zip(after, before)] == want


@pytest.mark.parametrize("B,T,n", [(3, 37, 4), (5, 13, 16)])
def test_unaligned_operands_take_the_runtime_body(wave_emu_backend, B, T, n):
    """Every operand a view offset by one float, and C_t out of a record whose slot is not 16-byte aligned: the scalar-load body,
    same bars."""
    before = launches(wave_emu_backend)
    cases.check("cpu", B, T, n, "shared", True, unaligned=True)
    cases.check("cpu", B, T, n, "packed", True, pad=3)
    assert [a - b for a, b in zip(launches(wave_emu_backend), before)] == [0, 0, 2, 2]


@pytest.mark.parametrize("B,T,n", [(2, 5, 4), (2, 4, 16)])
def test_joint_gaussian(wave_emu_backend, B, T, n):
    before = launches(wave_emu_backend)
    cases.joint_gaussian("cpu", B, T, n)
    assert launches(wave_emu_backend)[body_of(n)] == before[body_of(n)] + 1


@pytest.mark.parametrize("B,T,n", [(3, 5, 4), (2, 3, 16), (3, 5, 7)])
def test_partial_outputs_and_repeatability(wave_emu_backend, B, T, n):
    cases.partial_outputs("cpu", B, T, n)


@pytest.mark.parametrize("n", [4, 16, 5])
def test_ladder_level_per_item(wave_emu_backend, n):
    before = launches(wave_emu_backend)
    cases.ladder("cpu", n)
    assert launches(wave_emu_backend)[body_of(n)] == before[body_of(n)] + 1
    cases.ladder("cpu", n, impl="torch")


def test_c_entry_point_rejects(wave_emu_backend):
    cases.c_abi(wave_emu_backend, "cpu")


def test_unsupported_shapes_take_torch(wave_emu_backend):
    cases.unsupported_takes_torch("cpu")


def test_host_tensors_take_torch_without_a_backend():
    """Product behaviour on host tensors (no test backend): predictive falls back to torch, forcing the kernel raises."""
    from kvae import _native
    from kvae.kalman import lgssm_ops
    saved = _native._test_backend
    _native._set_test_backend(None)
    try:
        case = cases.inputs(2, 5, 4, "shared")
        k = case["k"]
        assert not lgssm_ops.predictive_supported(4, 2, k["Sp"])
        got = lgssm_ops.predictive(k["mp"], k["Sp"], k["C"], k["R"], k["Y"], k["mask"])
        assert all(v < cases.TOL[name] for name, v in cases.ratios(got, cases.reference(case)).items())
        with pytest.raises(RuntimeError):
            lgssm_ops.predictive(k["mp"], k["Sp"], k["C"], k["R"], k["Y"], k["mask"], impl="kernel")
    finally:
        _native._set_test_backend(saved)


# ---- model level ------------------------------------------------------------------------------------------------------------
_PATHS = {}


@pytest.mark.parametrize("kind,K", cases.MODELS)
def test_score(wave_emu_backend, kind, K):
    before = launches(wave_emu_backend)
    _, path = cases.model_score("cpu", kind, K)
    _PATHS[(kind, K)] = path
    assert launches(wave_emu_backend)[N4] > before[N4] and launches(wave_emu_backend)[SEQ] > before[SEQ]


@pytest.mark.parametrize("kind,K", cases.MODELS)
def test_log_likelihood(wave_emu_backend, kind, K):
    before = launches(wave_emu_backend)
    cases.model_log_likelihood("cpu", kind, K)
    assert launches(wave_emu_backend)[N4] > before[N4]


def test_model_yardsticks_are_what_float32_torch_gives(wave_emu_backend):
    """As above, for the model level: the float32 run of the restatement against its float64 run."""
    paths = dict(_PATHS)
    for kind, K in cases.MODELS:
        if kind == "switching" and (kind, K) not in paths:
            model = cases.small_model(kind, K)
            d = cases.model_inputs(model, K)
            paths[(kind, K)] = model.score(d["x"], u=d["u"], mask=d["mask"])["regimes"]
    got = cases.model_yardsticks(paths)
    print({k: float(f"{v:.3g}") for k, v in got.items()})
    for k, v in got.items():
        assert v / 3 <= cases.MODEL_YARDSTICK[k] <= v * 3, (k, v, cases.MODEL_YARDSTICK[k])


def test_prediction_scores(wave_emu_backend):
    cases.model_prediction_scores("cpu")
    cases.model_prediction_scores("cpu", "switching", 3)


def test_model_errors(wave_emu_backend):
    cases.model_errors("cpu")


def test_calibration(wave_emu_backend):
    before = launches(wave_emu_backend)
    wave_emu_backend.dll.kvae_hostsim_wave_emu(0)   # the filter of 64 x 128 steps on the plain host bodies; the predictive
    try:                                            # launches are emulated wavefronts either way
        cases.calibration("cpu")
    finally:
        wave_emu_backend.dll.kvae_hostsim_wave_emu(1)
    assert launches(wave_emu_backend)[N4] == before[N4] + 1


# ---- the gfx950 build and the sanitizers --------------------------------------------------------------------------------------
def test_kernels_have_no_scratch():
    """The resource report of every kernel of the unit (gfx950 cross-compile): 0 bytes of scratch per lane."""
    src = ROOT / "kalman-vae_amd" / "csrc" / "kvae_lgssm_pred.hip"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-amdgpu-mfma-vgpr-form", "-c",
                        str(src), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S*k_pred_\S*)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == 4 and len(scratch) == 4, (names, scratch)
    assert sum("k_pred_items" in n for n in names) == 3 and sum("k_pred_seq" in n for n in names) == 1
    assert all(s == 0 for s in scratch), list(zip(names, scratch))


def test_kernel_bodies_under_sanitizers():
    """A standalone driver of csrc/lgssm_pred.h on emulated wavefronts (tests/hostsim/pred_asan_driver.cpp), built with
    -fsanitize=address,undefined and run as a child process: all three bodies and the sequence sums, ragged B*T, T = 1, every
    buffer at its exact size."""
    out = ROOT / "tests" / "hostsim" / "pred_asan_driver"
    src = ROOT / "tests" / "hostsim" / "pred_asan_driver.cpp"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-fno-sanitize-recover=undefined", "-o", str(out), str(src)], check=True, cwd=ROOT)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(out)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "PRED-ASAN-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
