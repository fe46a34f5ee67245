"""CPU tier of kvae_lgssm_switching_viterbi / lgssm_ops.switching_viterbi / KalmanFilter.viterbi_regimes / KVAE.viterbi_regimes:
the host simulation injected (as tests/test_switching_filter.py does), so the kernel body of csrc/lgssm_swv.h runs on emulated
wavefronts (tests/hostsim/wave_emu.h); the launch counter says that it ran.  Against the float64 restatement per step
(tests/swv_cases.py), one Kalman filter along the returned path, the enumeration of every regime path, closed forms for P = I,
shared dynamics and K = 1, chunked streams, partial outputs, the C ABI, the model level, the resource report of the gfx950 kernel,
and the body under ASan + UBSan."""
import os
import re
import subprocess
from pathlib import Path

import pytest
import torch

import swv_cases as cases
from hostsim.build import build as build_hostsim

torch.set_num_threads(4)
ROOT = Path(__file__).resolve().parents[1]


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
    """emulated launches so far (csrc/lgssm_swv.h, KVAE_WAVE_EMU section): the sweep with its backtrace"""
    return lib.dll.kvae_wemu_switching_viterbi_launches(0)


@pytest.mark.parametrize("case", cases.CASES + [cases.LONG_CASE], ids=str)
def test_per_step_vs_float64(wave_emu_backend, case):
    before = launches(wave_emu_backend)
    cases.per_step("cpu", case)
    assert launches(wave_emu_backend) == before + 1


def test_yardsticks_are_what_float32_torch_gives():
    """The constants the bars derive from: the float32 restatement against the float64 one, remeasured.  Each is the largest of
    a few thousand rounding samples and moves with the host's vector width and libm: within a factor 3 either way."""
    for k, v in cases.yardsticks().items():
        assert v / 3 <= cases.YARDSTICK[k] <= v * 3, (k, v, cases.YARDSTICK[k])


def test_model_yardsticks_are_what_float32_torch_gives(wave_emu_backend):
    for k, v in cases.model_yardsticks().items():
        assert v / 3 <= cases.MODEL_YARDSTICK[k] <= v * 3, (k, v, cases.MODEL_YARDSTICK[k])


@pytest.mark.parametrize("case", cases.CASES + [cases.LONG_CASE], ids=str)
def test_score_of_the_path_is_exact_in_float64(case):
    cases.score_is_exact(case)


@pytest.mark.parametrize("case", cases.CASES + [cases.LONG_CASE], ids=str)
def test_score_and_beliefs_vs_the_pinned_filter(wave_emu_backend, case):
    before = launches(wave_emu_backend)
    cases.score_is_exact_on_kernel("cpu", case)
    assert launches(wave_emu_backend) == before + 1


@pytest.mark.parametrize("K,T", [(2, 1), (2, 2), (3, 1), (3, 2)])
def test_true_map_when_short(wave_emu_backend, K, T):
    cases.true_map_when_short("cpu", K, T)


@pytest.mark.parametrize("K,T", [(2, 6), (3, 5)])
def test_bounded_by_the_enumerated_map(wave_emu_backend, K, T):
    cases.bounded_by_the_map("cpu", K, T)


def test_identity_prior(wave_emu_backend):
    cases.identity_prior("cpu")


def test_shared_dynamics_take_regime_zero(wave_emu_backend):
    cases.shared_dynamics("cpu")


def test_single_regime_is_the_existing_filter(wave_emu_backend):
    cases.single_regime("cpu")


@pytest.mark.parametrize("case", [c for c in cases.CASES if c[5] and c[1] >= 8], ids=str)
def test_streaming_is_bit_identical(wave_emu_backend, case):
    cases.streaming("cpu", case)


def test_partial_outputs_and_repeatability(wave_emu_backend):
    before = launches(wave_emu_backend)
    cases.partial_outputs("cpu", (3, 5, 3, 4, 2, True))
    assert launches(wave_emu_backend) == before + 2 + 8   # two full calls, every output alone


def test_routing(wave_emu_backend):
    before = launches(wave_emu_backend)
    cases.routing("cpu")
    assert launches(wave_emu_backend) == before + 1   # only the last, supported, call


def test_host_tensors_take_the_restatement_without_a_backend(wave_emu_backend):
    from kvae import _native
    args, mask = cases.swf_cases.inputs(2, 4, 3)
    _native._set_test_backend(None)
    try:
        before = launches(wave_emu_backend)
        out = cases.run("cpu", args, mask)
        assert out["scores"].dtype == torch.float32 and launches(wave_emu_backend) == before
        assert cases.run("cpu", tuple(a.double() for a in args), mask)["scores"].dtype == torch.float64
        with pytest.raises(ValueError, match="impl='hip'"):
            cases.run("cpu", args, mask, impl="hip")
    finally:
        _native._set_test_backend(wave_emu_backend)


def test_c_abi(wave_emu_backend):
    cases.c_abi(wave_emu_backend, "cpu")


def test_model_level(wave_emu_backend):
    before = launches(wave_emu_backend)
    cases.model_level("cpu")
    assert launches(wave_emu_backend) > before


def test_model_errors(wave_emu_backend):
    cases.model_errors("cpu")


def test_viterbi_scores(wave_emu_backend):
    cases.viterbi_scores("cpu")


def test_kernels_have_no_scratch():
    """The resource report of every kernel of the unit (gfx950 cross-compile): 0 bytes of scratch per lane and no LDS."""
    src = ROOT / "kalman-vae_amd" / "csrc" / "kvae_lgssm_swv.hip"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-amdgpu-mfma-vgpr-form", "-c",
                        str(src), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S*k_swv_\S*)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(names) == 1 and len(scratch) == 1 and len(lds) == 1, (names, scratch, lds)
    assert "k_swv_sweep" in names[0]
    assert scratch == [0] and lds == [0], (names, scratch, lds)


def test_kernel_body_under_sanitizers():
    """A standalone driver of csrc/lgssm_swv.h (tests/hostsim/swv_asan_driver.cpp), built with -fsanitize=address,undefined and
    run as a child process: T = 1, K = 5 / 7 / 8, run-time n and m below 4, masks, NULL outputs, a carried state, T = 66."""
    out = ROOT / "tests" / "hostsim" / "swv_asan_driver"
    src = ROOT / "tests" / "hostsim" / "swv_asan_driver.cpp"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-fno-sanitize-recover=undefined", "-I", str(ROOT / "tests" / "hostsim" / "stub"), "-o", str(out), str(src)],
                   check=True, cwd=ROOT)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(out)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "SWV-ASAN-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
