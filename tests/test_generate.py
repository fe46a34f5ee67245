"""CPU tier of KVAE.generate: the host simulation injected (as tests/test_wave_emu.py does), so the rollout runs the kernel body
of csrc/lgssm_gen.h on emulated wavefronts (tests/hostsim/wave_emu.h).  Noise-free generation against the reference's impute
with the tail hidden (tests/golden/make_goldens_generate.py), the rollout with injected noise against an fp64 restatement
(tests/gen_cases.py: whole tensors, and per (rollout, step) up to 3073 rollouts), the structure of sampled regimes, argument errors, and the kernel body under ASan + UBSan."""
import ctypes
import os
import subprocess
from pathlib import Path

import pytest
import torch

import gen_cases
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


def gen_launches(lib):
    return lib.dll.kvae_wemu_generate_launches()   # emulated rollout launches (csrc/lgssm_gen.h, KVAE_WAVE_EMU section)


@pytest.mark.parametrize("name", ["gen_lstm_K1", "gen_lstm_K3", "gen_lstm_K7", "gen_lstm_K3_u"])
def test_noise_free_matches_reference_impute(wave_emu_backend, name):
    before = gen_launches(wave_emu_backend)
    gen_cases.golden_generate(name, "cpu")
    assert gen_launches(wave_emu_backend) > before   # the emulated kernel is what ran


@pytest.mark.parametrize("kind,K,n", [("lstm", 1, 4), ("lstm", 3, 4), ("lstm", 7, 4), ("lstm", 1, 16), ("lstm", 3, 16),
                                      ("lstm", 7, 16), ("lstm", 3, 5), ("switching", 3, 4), ("switching", 7, 16)])
def test_kernel_vs_restatement(wave_emu_backend, kind, K, n):
    """Injected noise, ragged R (B = 3, S = 7: 21 rollouts, 4 per wavefront), non-zero controls; n = 5 takes the run-time-
    dimension instantiation."""
    before = gen_launches(wave_emu_backend)
    pr = gen_cases.random_problem(kind, K, n, n, 2, B=3, S=7, H=3, seed=K * 31 + n)
    gen_cases.rollout_vs_restatement("cpu", pr)
    assert gen_launches(wave_emu_backend) > before


@pytest.mark.parametrize("kind,K,with_noise", [("lstm", 3, True), ("switching", 3, True), ("switching", 7, False),
                                               ("lstm", 3, False)])
def test_kernel_one_step(wave_emu_backend, kind, K, with_noise):
    """H = 1, one sequence, one sample; noise-free runs (NULL noise pointers) included."""
    pr = gen_cases.random_problem(kind, K, 4, 4, 2, B=1, S=1, H=1, seed=7 + K, with_noise=with_noise)
    gen_cases.rollout_vs_restatement("cpu", pr)


def test_torch_path_vs_restatement():
    """The torch rollout (alpha-network shapes outside the kernel) against the same restatement."""
    for kind, K, hidden in (("lstm", 3, 32), ("switching", 3, 50)):
        pr = gen_cases.random_problem(kind, K, 4, 4, 2, B=2, S=3, H=4, hidden=hidden, seed=3)
        gen_cases.rollout_vs_restatement("cpu", pr, impl="torch")


def test_switching_regimes(wave_emu_backend):
    """Sampled regimes are one-hot; with p_stay = 1 the regime never leaves the one it started in."""
    pr = gen_cases.random_problem("switching", 5, 4, 4, 2, B=3, S=5, H=6, seed=11)
    _, _, w = gen_cases.rollout_vs_restatement("cpu", pr)
    assert bool(((w == 0) | (w == 1)).all()) and bool((w.sum(-1) == 1).all())
    pr = gen_cases.random_problem("switching", 5, 4, 4, 2, B=3, S=5, H=6, seed=12, p_stay=1.0)
    _, _, w = gen_cases.rollout_vs_restatement("cpu", pr)
    start = pr["s0"][:, None, None, :].expand_as(w)
    assert torch.equal(w, start)


def test_restate_vec_is_restate():
    """The side-by-side float64 form of the restatement (the reference at thousands of rollouts) IS the scalar one: 1e-12."""
    for c in gen_cases.GEN_CASES[:22]:
        pr = gen_cases.gen_case_problem(c)
        for x, y in zip(gen_cases.restate(pr, torch.float64), gen_cases.restate_vec(pr, torch.float64)):
            assert x.shape == y.shape and float((x - y).abs().max()) <= 1e-12, gen_cases.gen_case_id(c)


def test_per_step_case_lists_reach_every_edge():
    """What the lists of rollout_per_step promise: every dispatch with K = 1, 2, 3, 16; every (B, S) of the quad; H = 1, 2, 3, 8;
    p = 1, 2, 3, 16; controls present and absent; every noise subset; 3072 and 3073 rollouts on each of the four instantiations."""
    cs = gen_cases.GEN_CASES
    assert {(c["kind"], c["n"], c["m"], c["K"]) for c in cs} == {d + (K,) for d in gen_cases.GEN_DISPATCHES for K in (1, 2, 3, 16)}
    assert {(c["B"], c["S"]) for c in cs} == set(gen_cases.GEN_BS) and {c["H"] for c in cs} == {1, 2, 3, 8}
    assert {c["p"] for c in cs} == {1, 2, 3, 16} and {c["with_u"] for c in cs} == {True, False}
    for kind, names in (("lstm", {"none", "eps0", "eps_z", "eps_a", "all"}), ("switching", {"none", "eps0", "gumbel", "eps_a", "all"})):
        assert {c["noise"] for c in cs if c["kind"] == kind} == names
        assert {c["with_u"] for c in cs if c["kind"] == kind} == {True, False}
    assert {c["p"] for c in cs if c["kind"] == "switching"} == {1, 3, 16} == {c["p"] for c in cs if c["kind"] == "lstm" and c["K"] == 1}
    fams = {(gen_cases.gen_family(c["kind"], c["n"], c["m"]), c["B"] * c["S"]) for c in gen_cases.GEN_LARGE_CASES}
    assert fams >= {(f, R) for f in ("lstm4", "lstm16", "rt", "sw") for R in (3072, 3073)}
    assert all(gen_cases.GEN_STEP_TOL[k] == 4.0 * v and v > 0 for k, v in gen_cases.GEN_YARDSTICK.items())


@pytest.mark.parametrize("case", gen_cases.GEN_CASES, ids=gen_cases.gen_case_id)
def test_rollout_per_step(wave_emu_backend, case):
    """Every (rollout, step) of a, z, weights against the float64 restatement under GEN_STEP_TOL; guards, sentinels, exact
    regimes, isolation of the sequences (gen_cases.rollout_per_step, which also asserts that the emulated kernel ran)."""
    print(gen_cases.run_gen_case("cpu", case))


@pytest.mark.parametrize("case", gen_cases.GEN_LARGE_CASES, ids=gen_cases.gen_case_id)
def test_rollout_per_step_many_rollouts(wave_emu_backend, case):
    """3072 rollouts (the last size at 4 per wavefront) and 3073 (8 per wavefront, the last one ragged) on every instantiation."""
    print(gen_cases.run_gen_case("cpu", case))


def small_model(kind="lstm", K=3, **kw):
    from kvae.model.model import KVAE
    from kvae.utils.config import KVAEConfig
    torch.manual_seed(0)
    return KVAE(KVAEConfig(dynamics_model=kind, num_modes=K, scheduled_beta=False, **kw))


def test_generate_model_level(wave_emu_backend):
    """Shapes, training mode and parameters left unchanged, a switching model end to end, conditioning mask."""
    for kind in ("lstm", "switching"):
        model = small_model(kind)
        model.train()
        before = {k: v.clone() for k, v in model.state_dict().items()}
        x = (torch.rand(2, 3, 1, 32, 32) > 0.7).float()
        mask = torch.tensor([[1.0, 0.0, 1.0], [1.0, 1.0, 0.0]])
        out = model.generate(x, 4, num_samples=3, mask=mask)
        assert out["a"].shape == (2, 3, 4, 2) and out["z"].shape == (2, 3, 4, 4) and out["weights"].shape == (2, 3, 4, 3)
        assert out["x"].shape == (2, 3, 4, 1, 32, 32) and out["a_vae"].shape == (2, 3, 2)
        assert model.training
        after = model.state_dict()
        assert all(torch.equal(before[k], after[k]) for k in before)
        assert model.generate(x, 2, decode=False)["x"] is None


def test_generate_argument_errors(wave_emu_backend):
    model = small_model()
    x = torch.zeros(2, 3, 1, 32, 32)
    with pytest.raises(ValueError):
        model.generate(x, 0)
    with pytest.raises(ValueError):
        model.generate(x, 2, num_samples=0)
    with pytest.raises(ValueError):
        model.generate(x, 2, u=torch.zeros(2, 4, 4))   # T0 + H = 5 steps needed
    with pytest.raises(ValueError):
        model.generate(x, 2, u=torch.zeros(2, 5, 3))


def test_c_entry_point_rejects(wave_emu_backend):
    """KVAE_ERR_DIMS for dims out of range, KVAE_ERR_NULL for missing required pointers, KVAE_ERR_ARG for a bad kind."""
    from kvae import _native as N
    buf = torch.zeros(4096)
    ptr = buf.data_ptr()

    def prob(**kw):
        pr = N.GenProblem()
        pr.B, pr.S, pr.H, pr.n, pr.m, pr.p, pr.K, pr.kind, pr.hidden = 1, 1, 1, 4, 4, 2, 1, 0, 50
        for k in ("A", "Bm", "C", "mu", "a_out", "z_out", "w_out"):
            setattr(pr, k, ptr)
        for k, v in kw.items():
            setattr(pr, k, v)
        return pr

    call = lambda pr: wave_emu_backend.dll.kvae_lgssm_generate(ctypes.byref(pr), None)
    assert call(prob()) == 0
    for kw in (dict(n=0), dict(n=17), dict(m=0), dict(p=17), dict(K=0), dict(K=17), dict(H=0), dict(B=0), dict(S=0),
               dict(K=3, hidden=32), dict(K=3, p=3)):
        assert call(prob(**kw)) == 1, kw
    for kw in (dict(A=None), dict(mu=None), dict(a_out=None), dict(w_out=None), dict(eps_z=ptr), dict(eps0=ptr),
               dict(K=3), dict(kind=1)):
        assert call(prob(**kw)) == 2, kw
    assert call(prob(kind=2)) == 4
    assert call(prob(kind=1, P=ptr, s0=ptr, eps_z=ptr, LQ=ptr)) == 4   # switching noise needs one-hot regimes
    assert wave_emu_backend.dll.kvae_lgssm_generate(None, None) == 2


def test_kernel_body_under_sanitizers():
    """A standalone driver of csrc/lgssm_gen.h on emulated wavefronts (tests/hostsim/gen_asan_driver.cpp), built with
    -fsanitize=address,undefined and run as a child process: a small lstm and a small switching case, ragged R."""
    out = ROOT / "tests" / "hostsim" / "gen_asan_driver"
    src = ROOT / "tests" / "hostsim" / "gen_asan_driver.cpp"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-fno-sanitize-recover=undefined", "-o", str(out), str(src)], check=True, cwd=ROOT)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(out)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "GEN-ASAN-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
