"""CPU tier of kvae_lgssm_switching_pf / lgssm_ops.switching_pf / KalmanFilter.particle_filter_regimes /
KVAE.particle_filter_regimes: the host simulation injected (as tests/test_switching_filter.py does), so the kernel bodies of
csrc/lgssm_spf.h run on emulated workgroups (tests/hostsim/wave_emu.h); the launch counters say which body ran.  Against the
float64 restatement replaying the kernel's decisions (tests/spf_cases.py), the decisions against the free-running float64 run,
the enumeration of every regime path (exactness and unbiasedness), the existing filter, lineages, chunked streams, partial
outputs, the C ABI, the model level, the resource report of the gfx950 kernels, and the bodies under ASan + UBSan."""
import os
import re
import subprocess
from pathlib import Path

import pytest
import torch

import spf_cases as cases
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
    """emulated launches so far (csrc/lgssm_spf.h, KVAE_WAVE_EMU section): [the sweep, the lineages, the sequence sums]"""
    return [lib.dll.kvae_wemu_switching_pf_launches(i) for i in (0, 1, 2)]


@pytest.mark.parametrize("case", cases.CASES + [cases.LONG_CASE], ids=str)
def test_per_step_vs_float64(wave_emu_backend, case):
    before = launches(wave_emu_backend)
    cases.per_step("cpu", case)
    assert [a - b for a, b in zip(launches(wave_emu_backend), before)] == [1, 1, 1]


def test_yardsticks_are_what_float32_torch_gives():
    """The constants the bars derive from: the float32 restatement against the float64 one under the same replayed decisions,
    remeasured.  Each is the largest of a few thousand rounding samples and moves with the host's vector width and libm: within a
    factor 3 either way."""
    for k, v in cases.yardsticks().items():
        assert v / 3 <= cases.YARDSTICK[k] <= v * 3, (k, v, cases.YARDSTICK[k])
    v = cases.identity_yardstick()
    assert v / 3 <= cases.IDENTITY_LOG_W <= v * 3, (v, cases.IDENTITY_LOG_W)


def test_model_yardsticks_are_what_float32_torch_gives(wave_emu_backend):
    for k, v in cases.model_yardsticks().items():
        assert v / 3 <= cases.MODEL_YARDSTICK[k] <= v * 3, (k, v, cases.MODEL_YARDSTICK[k])


@pytest.mark.parametrize("case", cases.CASES + [cases.LONG_CASE], ids=str)
def test_few_reference_decisions_fall_under_their_margins(case):
    cases.margins_hold(case)


@pytest.mark.parametrize("case", cases.CASES + [cases.LONG_CASE], ids=str)
def test_restatement_is_exact_at_step_zero(case):
    cases.first_step_is_exact(case)


def test_restatement_is_exact_for_shared_dynamics():
    cases.exact_shared_dynamics()


def test_restatement_with_one_regime_is_the_single_filter_in_float64():
    cases.exact_single_regime()


def test_restatement_reaches_every_ladder_level():
    cases.ladder_levels(None)


def test_every_ladder_level_on_the_kernel(wave_emu_backend):
    before = launches(wave_emu_backend)
    cases.ladder_levels("cpu")
    assert launches(wave_emu_backend)[0] == before[0] + 1


def test_restatement_under_an_identity_prior():
    cases.identity_prior(None)


def test_identity_prior_on_the_kernel(wave_emu_backend):
    before = launches(wave_emu_backend)
    cases.identity_prior("cpu")
    assert launches(wave_emu_backend)[0] == before[0] + 2


@pytest.mark.parametrize("thr", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("K", [1, 3])
def test_identical_regimes_are_the_existing_filter(wave_emu_backend, K, thr):
    before = launches(wave_emu_backend)
    cases.vs_existing_filter("cpu", K, thr)
    assert launches(wave_emu_backend)[0] == before[0] + 1


@pytest.mark.parametrize("thr", [0.5, 1.0])
@pytest.mark.parametrize("K,T", [(2, 10), (3, 8)])
def test_unbiased_on_the_emulated_kernel(wave_emu_backend, K, T, thr):
    """The GPU tier runs the 512 replicates the check is specified with; the emulated workgroups take 64 (the 5 standard errors
    are those of the replicates there are)."""
    before = launches(wave_emu_backend)
    cases.unbiased("cpu", K, T, thr, G=64)
    assert launches(wave_emu_backend)[0] == before[0] + 1


@pytest.mark.parametrize("thr", [0.5, 1.0])
@pytest.mark.parametrize("K,T", [(2, 10), (3, 8)])
def test_restatement_is_unbiased(K, T, thr):
    cases.unbiased("cpu", K, T, thr, G=512, impl="torch")


def test_lineages(wave_emu_backend):
    before = launches(wave_emu_backend)
    cases.lineage_rules("cpu")
    assert [a - b for a, b in zip(launches(wave_emu_backend), before)][:2] == [2, 2]


@pytest.mark.parametrize("case", [c for c in cases.CASES if c[6] and c[2] >= 8], ids=str)
def test_streaming_is_bit_identical(wave_emu_backend, case):
    cases.streaming("cpu", case)


def test_partial_outputs_and_repeatability(wave_emu_backend):
    before = launches(wave_emu_backend)
    cases.partial_outputs("cpu", (3, 3, 5, 3, 4, 2, False, 64, 0.5))
    # every output sweeps (log_lik_seq reads log_lik, paths read regimes and ancestors)
    assert [a - b for a, b in zip(launches(wave_emu_backend), before)] == [2 + 13, 2 + 1, 2 + 1]


def test_routing(wave_emu_backend):
    before = launches(wave_emu_backend)
    cases.routing("cpu")
    assert [a - b for a, b in zip(launches(wave_emu_backend), before)] == [1, 1, 1]   # only the last, supported, call


def test_host_tensors_raise_without_a_backend(wave_emu_backend):
    """fp32 host tensors of a supported shape are not routed to the kernel when no test backend is injected: they take the
    restatement, as float64 ones do; impl="hip" raises."""
    from kvae import _native
    case = (2, 2, 3, 2, 4, 2, False, 64, 0.5)
    args, mask, th, ph, _ = cases.reference(case)
    _native._set_test_backend(None)
    try:
        before = launches(wave_emu_backend)
        out = cases.run("cpu", args, th, ph, mask)
        assert out["regime_filt"].dtype == torch.float32 and launches(wave_emu_backend) == before
        assert cases.run("cpu", tuple(a.double() for a in args), th, ph, mask)["regime_filt"].dtype == torch.float64
        with pytest.raises(ValueError, match="impl='hip'"):
            cases.run("cpu", args, th, ph, mask, impl="hip")
    finally:
        _native._set_test_backend(wave_emu_backend)


def test_c_abi(wave_emu_backend):
    cases.c_abi(wave_emu_backend, "cpu")


def test_model_level(wave_emu_backend):
    before = launches(wave_emu_backend)
    cases.model_level("cpu")
    assert launches(wave_emu_backend)[0] > before[0]


def test_model_errors(wave_emu_backend):
    before = launches(wave_emu_backend)
    cases.model_errors("cpu")
    assert launches(wave_emu_backend) == before


def test_particle_filter_scores(wave_emu_backend):
    cases.pf_scores("cpu")


def test_noise_slots_default_to_none():
    from kvae import noise
    assert noise.take("pf_regime") is None and noise.take("pf_resample") is None
    u = noise.uniform("pf_regime", (2, 3), "cpu", torch.float32)
    assert u.shape == (2, 3) and bool((u >= 0).all()) and bool((u < 1).all())
    with noise.inject(pf_resample=torch.full((6,), 0.25)):
        assert bool((noise.uniform("pf_resample", (2, 3), "cpu", torch.float64) == 0.25).all())
    assert noise.take("pf_resample") is None


def test_kernels_have_no_scratch():
    """The resource report of every kernel of the unit (gfx950 cross-compile): 0 bytes of scratch per lane; LDS only in the
    sweep (the dynamics tables, the reduction rows, the scan and the resampling stage: 18 KB, so LDS never limits occupancy
    before the registers do)."""
    src = ROOT / "kalman-vae_amd" / "csrc" / "kvae_lgssm_spf.hip"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-amdgpu-mfma-vgpr-form", "-c",
                        str(src), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S*k_spf_\S*)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(names) == 3 and len(scratch) == 3 and len(lds) == 3, (names, scratch, lds)
    assert all(s == 0 for s in scratch), list(zip(names, scratch))
    by_name = dict(zip(names, lds))
    for name, v in by_name.items():
        if "k_spf_sweep" in name:
            assert 0 < v <= 20 * 1024, (name, v)
        else:
            assert v == 0, (name, v)


def test_kernel_body_under_sanitizers():
    """A standalone driver of csrc/lgssm_spf.h (tests/hostsim/spf_asan_driver.cpp), built with -fsanitize=address,undefined and
    run as a child process: T = 1, K = 5 / 7 / 8, run-time n and m below 4, masks, NULL outputs, a carried state, N = 64 and
    256, ess_threshold 0 / 0.5 / 1, T = 66."""
    out = ROOT / "tests" / "hostsim" / "spf_asan_driver"
    src = ROOT / "tests" / "hostsim" / "spf_asan_driver.cpp"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-fno-sanitize-recover=undefined", "-I", str(ROOT / "tests" / "hostsim" / "stub"), "-o", str(out), str(src)],
                   check=True, cwd=ROOT)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(out)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "SPF-ASAN-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
