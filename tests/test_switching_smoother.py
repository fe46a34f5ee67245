"""CPU tier of kvae_lgssm_switching_smoother / lgssm_ops.switching_smoother / KalmanFilter.smooth_regimes / KVAE.smooth_regimes:
the host simulation injected (as tests/test_switching_filter.py does), so the kernel bodies of csrc/lgssm_swf.h (the forward, with
its history kept) and csrc/lgssm_sws.h (the backward) run on emulated wavefronts (tests/hostsim/wave_emu.h); the launch counters
say which body ran.  Against the float64 restatement per (b, t) (tests/sws_cases.py), references independent of it (one smoother
per regime, every path enumerated), the existing smoother, partial outputs, the C ABI, the model level, the resource report of the
gfx950 kernels, and the bodies under ASan + UBSan."""
import os
import re
import subprocess
from pathlib import Path

import pytest
import torch

import sws_cases as cases
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
    """emulated launches so far (csrc/lgssm_sws.h, KVAE_WAVE_EMU section): [the forward, the backward, the sequence sums]"""
    return [lib.dll.kvae_wemu_switching_smoother_launches(i) for i in (0, 1, 2)]


def delta(lib, before):
    return [a - b for a, b in zip(launches(lib), before)]


@pytest.mark.parametrize("case", cases.CASES + [cases.LONG_CASE], ids=str)
def test_per_step_vs_float64(wave_emu_backend, case):
    """The closest: Sigmas_smooth of the long case (2, 70, 7), 9.6e-6 against the bar of 1.02e-5 on the host simulation (gfx950:
    5.3e-6), at the one step where the regime changes.  Its mus_smooth is 2.5e-6 against 5.2e-6 because the backward body
    divides M_{t+1}(g) by the column sum of W_{t+1} (1 in exact arithmetic); with the plain product the total regime mass
    drifted by 1e-6 over the 70 steps and mus_smooth was 6.07e-6 ("The column sum")."""
    before = launches(wave_emu_backend)
    cases.per_step("cpu", case)
    assert delta(wave_emu_backend, before) == [1, 1, 1]


def test_yardsticks_are_what_float32_torch_gives():
    """The constants the bars derive from: the float32 restatement against the float64 one, remeasured.  Each is the largest of
    a few hundred rounding samples and moves with the host's vector width and libm: within a factor 3 either way."""
    for k, v in cases.yardsticks().items():
        assert v / 3 <= cases.YARDSTICK[k] <= v * 3, (k, v, cases.YARDSTICK[k])


def test_model_yardsticks_are_what_float32_torch_gives(wave_emu_backend):
    for k, v in cases.model_yardsticks().items():
        assert v / 3 <= cases.MODEL_YARDSTICK[k] <= v * 3, (k, v, cases.MODEL_YARDSTICK[k])


def test_reference_decides_every_regime():
    cases.reference_leaves_no_regime_out()


def test_restatement_is_exact_under_an_identity_prior():
    cases.exact_identity_prior()


def test_restatement_is_exact_for_shared_dynamics():
    cases.exact_shared_dynamics()


@pytest.mark.parametrize("K", [2, 3])
def test_restatement_regimes_are_exact_at_two_steps(K):
    cases.exact_two_steps(K)


def test_pair_marginals_sum_to_the_regime_marginals():
    cases.pair_sums()


def test_hard_prior_is_finite():
    cases.hard_prior_is_finite()


def test_hard_prior_on_the_kernel(wave_emu_backend):
    before = launches(wave_emu_backend)
    cases.hard_prior_on_kernel("cpu")
    assert delta(wave_emu_backend, before)[:2] == [1, 1]


@pytest.mark.parametrize("K", [1, 3])
def test_identical_regimes_are_the_existing_smoother(wave_emu_backend, K):
    before = launches(wave_emu_backend)
    cases.vs_existing_smoother("cpu", K)
    assert delta(wave_emu_backend, before)[:2] == [1, 1]


def test_single_step_is_the_filter(wave_emu_backend):
    cases.single_step("cpu")


def test_partial_outputs_and_repeatability(wave_emu_backend):
    before = launches(wave_emu_backend)
    cases.partial_outputs("cpu", (3, 5, 3, 4, 2, True))
    # two full calls, four single outputs, the mixed call: forward and backward; the filter-only call: no backward
    assert delta(wave_emu_backend, before) == [8, 7, 3]


def test_carried_state(wave_emu_backend):
    cases.carried_state("cpu")


def test_routing(wave_emu_backend):
    before = launches(wave_emu_backend)
    cases.routing("cpu")
    assert delta(wave_emu_backend, before) == [1, 1, 1]   # only the last, supported, call


def test_c_abi(wave_emu_backend):
    cases.c_abi(wave_emu_backend, "cpu")


def test_model_level(wave_emu_backend):
    before = launches(wave_emu_backend)
    cases.model_level("cpu")
    assert delta(wave_emu_backend, before)[:2] == [3, 3]


def test_model_errors(wave_emu_backend):
    before = launches(wave_emu_backend)
    cases.model_errors("cpu")
    assert launches(wave_emu_backend) == before


def test_regime_smoother_scores(wave_emu_backend):
    cases.smoother_scores("cpu")


def test_kernels_have_no_scratch():
    """The resource report of every kernel of the unit (gfx950 cross-compile): 0 bytes of scratch per lane, no LDS."""
    src = ROOT / "kalman-vae_amd" / "csrc" / "kvae_lgssm_sws.hip"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-amdgpu-mfma-vgpr-form", "-c",
                        str(src), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S*k_sws_\S*)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(names) == 3 and len(scratch) == 3 and len(lds) == 3, (names, scratch, lds)
    assert any("k_sws_fwd" in n for n in names) and any("k_sws_back" in n for n in names)
    assert all(s == 0 for s in scratch), list(zip(names, scratch))
    assert all(v == 0 for v in lds), list(zip(names, lds))


def test_kernel_bodies_under_sanitizers(tmp_path):
    """A standalone driver of csrc/lgssm_sws.h (tests/hostsim/sws_asan_driver.cpp), built with -fsanitize=address,undefined into
    a temporary directory and run as a child process: T = 1 and 2, K = 5, 7, 8 (padding lanes and a full grid), run-time n = 3
    and m = 1, a mask, NULL outputs, a carried state, T = 66, the error codes."""
    out = tmp_path / "sws_asan_driver"
    src = ROOT / "tests" / "hostsim" / "sws_asan_driver.cpp"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-fno-sanitize-recover=undefined", "-I", str(ROOT / "tests" / "hostsim" / "stub"), "-o", str(out), str(src)],
                   check=True, cwd=ROOT)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(out)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "SWS-ASAN-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
