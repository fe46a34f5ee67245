"""CPU tier of KalmanFilter.sample_posterior / KVAE.sample_imputations: the host simulation injected (as tests/test_generate.py
does), so the gains and the paths run the kernel bodies of csrc/lgssm_post.h on emulated wavefronts (tests/hostsim/wave_emu.h).
Pinned to the reference's masked fixtures (noise-free paths, moments of sampled paths), against an fp64 restatement
(tests/post_cases.py: whole tensors, and per gains item / per (path, step)), the per-item Cholesky ladder, the model level against KVAE.impute, argument errors, the resource report
of the gfx950 kernels, and both kernel bodies under ASan + UBSan."""
import ctypes
import os
import re
import subprocess
from pathlib import Path

import pytest
import torch

import post_cases
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
    return lib.dll.kvae_wemu_posterior_launches()   # emulated calls (csrc/lgssm_post.h, KVAE_WAVE_EMU section)


@pytest.mark.parametrize("name,kind", post_cases.FIXTURES)
def test_noise_free_matches_reference_smoother(wave_emu_backend, name, kind):
    before = launches(wave_emu_backend)
    post_cases.golden_noise_free(name, kind, "cpu")
    assert launches(wave_emu_backend) > before   # the emulated kernels are what ran


@pytest.mark.parametrize("name,kind", post_cases.FIXTURES)
def test_moments_match_reference_smoother(wave_emu_backend, name, kind):
    """S = 8192 paths, seed 1, over the fixture's own filter stacks: sample mean, covariance and lag-one cross-covariance within
    5 standard errors of mus_smooth, Sigmas_smooth and J_t Sigma_{t+1|T} at every (b, t, i, j).  (An fp64 and an fp32 torch
    restatement fed these draws stay at or below 1.54 / 2.13 / 2.13 s.e. on the lstm fixture and 2.61 / 2.32 / 2.19 on the
    switching one.)  Independent per-step draws would pass the first two and fail the third."""
    before = launches(wave_emu_backend)
    e_mean, e_cov, e_lag = post_cases.golden_moments(name, "cpu")
    assert e_mean <= 5 and e_cov <= 5 and e_lag <= 5, (e_mean, e_cov, e_lag)
    assert launches(wave_emu_backend) > before


def test_moments_detect_incoherent_paths():
    """The lag check is what tells joint samples from per-step marginal draws: z_t = mu_{t|T} + chol(Sigma_{t|T}) eps_t has the
    right means and covariances and no lag-one cross-covariance."""
    g = post_cases.load(post_cases.FIXTURES[0][0])
    eps = torch.randn(2, 8192, 100, 4, generator=torch.Generator().manual_seed(1))
    L = torch.linalg.cholesky(g["Sigmas_smooth"].double())
    z = g["mus_smooth"].squeeze(-1).double()[:, None] + (L[:, None] @ eps.double().unsqueeze(-1)).squeeze(-1)
    e_mean, e_cov, e_lag = post_cases.moment_errors(z, g)
    assert e_mean <= 5 and e_cov <= 5 and e_lag > 5, (e_mean, e_cov, e_lag)


@pytest.mark.parametrize("n,per_step_Q", [(4, True), (4, False), (16, True), (16, False), (5, True), (5, False)])
def test_kernels_vs_restatement(wave_emu_backend, n, per_step_Q):
    """Ragged sizes (B = 3, S = 7, T = 9: 27 items, 21 paths); n = 5 takes the run-time-dimension instantiations."""
    before = launches(wave_emu_backend)
    pr = post_cases.random_problem(n, 2, B=3, S=7, T=9, seed=10 * n + per_step_Q, per_step_Q=per_step_Q)
    post_cases.paths_vs_restatement("cpu", pr, want_levels=[0])
    assert launches(wave_emu_backend) > before


@pytest.mark.parametrize("n,p,B,S,T,kw", [
    (4, 2, 2, 70, 5, {}),                                   # more than one wavefront per sequence
    (16, 3, 1, 70, 3, {}),
    (4, 2, 3, 5, 1, {}),                                    # T = 1: only the start
    (16, 2, 2, 3, 1, {}),
    (4, 2, 3, 5, 2, {}),                                    # T = 2
    (5, 3, 2, 4, 2, {}),
    (4, 2, 5, 1, 6, {}),                                    # S = 1
    (16, 2, 2, 1, 4, {}),
    (4, 2, 3, 4, 6, dict(with_noise=False)),                # noise-free: NULL pointers
    (16, 2, 2, 3, 4, dict(with_noise=False)),
    (4, 2, 3, 4, 6, dict(emission_noise=True)),             # emission noise on
    (16, 5, 2, 3, 4, dict(emission_noise=True)),
    (7, 16, 2, 3, 4, dict(emission_noise=True)),
    (4, 2, 2, 3, 5, dict(with_noise=False, emission_noise=True)),
])
def test_kernels_shapes(wave_emu_backend, n, p, B, S, T, kw):
    pr = post_cases.random_problem(n, p, B=B, S=S, T=T, seed=n + p + B + S + T, **kw)
    post_cases.paths_vs_restatement("cpu", pr, want_levels=[0])


@pytest.mark.parametrize("n", [4, 16, 5])
def test_packed_record_is_bit_identical(wave_emu_backend, n):
    """A | C | Q read from the slots of one packed step record vs the same problem as plain tensors."""
    pr = post_cases.random_problem(n, 2, B=3, S=5, T=6, seed=40 + n, emission_noise=True)
    plain = post_cases.run_paths("cpu", pr)
    rec, slots = post_cases.pack_record(pr)
    packed = post_cases.run_paths("cpu", pr, packed=rec, slots=slots)
    for x, y in zip(plain, packed):
        assert torch.equal(x, y)


@pytest.mark.parametrize("n", [4, 16, 5])
def test_stages_gains_once_paths_again(wave_emu_backend, n):
    """The gains launch alone, then the path launch alone (twice, the second with other draws): the same bits as one call."""
    from kvae.kalman import lgssm_ops
    pr = post_cases.random_problem(n, 2, B=3, S=5, T=6, seed=70 + n)
    whole = post_cases.run_paths("cpu", pr)
    call = lgssm_ops.PosteriorCall(**pr)
    call.z.fill_(float("nan"))
    call.run(call.GAINS)
    assert bool(torch.isnan(call.z).all()) and torch.equal(call.levels, whole[2])
    call.run(call.PATHS)
    assert torch.equal(call.z, whole[0]) and torch.equal(call.a, whole[1])
    other = dict(pr, eps=torch.randn(3, 5, 6, n, generator=torch.Generator().manual_seed(9)))
    call.new_draws(eps=other["eps"])
    call.run(call.PATHS)
    want = post_cases.run_paths("cpu", other)
    assert torch.equal(call.z, want[0]) and torch.equal(call.a, want[1])


@pytest.mark.parametrize("n", [4, 16])
def test_misaligned_operands_take_the_fallback(wave_emu_backend, n):
    """Draws and filter stacks 4 bytes off a 16-byte boundary: the scalar-load instantiation, same results."""
    pr = post_cases.random_problem(n, 2, B=3, S=5, T=6, seed=50 + n)
    aligned = post_cases.run_paths("cpu", pr)

    def shift(t):
        buf = torch.empty(t.numel() + 5)
        off = 1 + ((16 - buf.data_ptr() % 16) % 16) // 4   # one float past a 16-byte boundary
        v = buf[off:off + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v

    off = dict(pr, **{k: shift(pr[k]) for k in ("eps", "Sigmas_filt", "Sigmas_pred", "A", "Cm", "Q")})
    got = post_cases.run_paths("cpu", off)
    post_cases.paths_vs_restatement("cpu", pr, got=got)
    for x, y in zip(aligned, got):
        assert float((x - y).abs().max()) <= 1e-5


def test_torch_path_vs_restatement():
    """The torch recursion against the same restatement, and an unsupported dtype takes it without error."""
    from kvae.kalman import lgssm_ops
    for n, kw in ((4, {}), (16, dict(per_step_Q=False)), (5, dict(emission_noise=True)), (4, dict(with_noise=False))):
        pr = post_cases.random_problem(n, 2, B=3, S=4, T=7, seed=60 + n, **kw)
        post_cases.paths_vs_restatement("cpu", pr, impl="torch", want_levels=[0])
    pr = post_cases.random_problem(4, 2, B=2, S=3, T=5, seed=3)
    p64 = {k: (v.double() if isinstance(v, torch.Tensor) else v) for k, v in pr.items()}
    assert not lgssm_ops.posterior_supported(4, 2, p64["Sigmas_filt"])
    z, a, lv = lgssm_ops.posterior_paths(**p64)
    ref = post_cases.restate(pr, torch.float64)
    assert z.dtype == torch.float64 and float((z - ref[0]).abs().max()) < 1e-9 and float((a - ref[1]).abs().max()) < 1e-9


def test_ladder_levels_per_item(wave_emu_backend):
    """One negative eigenvalue in Sigma_{t|t} at chosen steps: levels 2, 3, 4 and the clamped diagonal, per item, as the
    restatement's; z finite and within the restatement bar; the torch path likewise."""
    before = launches(wave_emu_backend)
    post_cases.check_ladder("cpu")
    assert launches(wave_emu_backend) > before
    post_cases.check_ladder("cpu", impl="torch")


def test_restate_paths_vec_is_restate():
    """The side-by-side float64 form of the path recursion (the reference of paths_per_step) IS the scalar restatement: 1e-12."""
    for c in post_cases.POST_RING_CASES[20:30] + post_cases.POST_SHAPE_CASES[-6:]:
        pr = post_cases.post_case_problem(c)
        ref = post_cases.restate(pr, torch.float64)
        for x, y in zip(post_cases.restate_paths_vec(pr, torch.float64), ref[:2]):
            assert x.shape == y.shape and float((x - y).abs().max()) <= 1e-12, post_cases.post_case_id(c)


def test_per_step_case_lists_reach_every_edge():
    """What the lists of gains_per_item / paths_per_step promise, and the bars: 4 x the tabled yardsticks."""
    ring = post_cases.POST_RING_CASES
    assert {(c["n"], c["misalign"], c["T"]) for c in ring} == {(n, mis, T) for n, mis in ((4, None), (16, None), (5, None), (4, "eps"), (16, "ws"))
                                                            for T in range(1, 10)}
    sh = post_cases.POST_SHAPE_CASES
    assert {c["B"] * c["S"] for c in sh if c["n"] == 4} >= {63, 64, 65} <= {c["B"] * c["S"] for c in sh if c["n"] == 5}
    assert {(c["B"], c["S"]) for c in sh if c["n"] == 16} >= {(1, 3), (2, 2), (5, 1), (3, 3), (2, 70)} and any((c["B"], c["S"]) == (5, 13) for c in sh)
    every = ring + sh
    for n in (4, 16, 5):
        mine = [c for c in every if c["n"] == n]
        assert {c["S"] for c in mine} >= {1, 70} and {c["per_step_Q"] for c in mine} == {True, False} == {c["shared_ac"] for c in mine}
        assert {c["with_noise"] for c in mine} == {True, False} == {c["rescaled"] for c in mine}
    assert {(c["p"], c["emission_noise"]) for c in every} >= {(p, e) for p in (1, 2, 3, 16) for e in (True, False)}
    c = post_cases.POST_EMIT_CASE
    assert c["B"] * c["S"] * c["T"] > 64 * 1024 and c["n"] == 4
    assert post_cases.POST_YARDSTICK and all(post_cases.POST_STEP_TOL[k] == 4.0 * v and v > 0 for k, v in post_cases.POST_YARDSTICK.items())


@pytest.mark.parametrize("case", post_cases.POST_GAIN_CASES, ids=post_cases.post_case_id)
def test_gains_per_item(wave_emu_backend, case):
    """The record J | L | c of every (b, t) against the float64 restatement under POST_STEP_TOL; levels, the triangle of L, J of
    the last item, guards and sentinels; the rescaled problems exchange rows at every item (post_cases.gains_per_item, which
    also asserts that the emulated kernels ran)."""
    print(post_cases.run_gain_case("cpu", case))


@pytest.mark.parametrize("name", list(post_cases.LADDER_CASES))
def test_ladder_per_item(wave_emu_backend, name):
    """Raised ladder levels at n = 4, 16 and 5, four different ones in one wavefront of the n = 4 gains, and one on the last
    item of a ragged last wavefront: levels as the float64 run's, L, z, a per slice under the .lv bars."""
    print(post_cases.ladder_per_item("cpu", name))


@pytest.mark.parametrize("case", post_cases.POST_RING_CASES + post_cases.POST_SHAPE_CASES, ids=post_cases.post_case_id)
def test_paths_per_step(wave_emu_backend, case):
    """z and a of every (path, step) against the float64 restatement under POST_STEP_TOL, a against the emission of the kernel's
    own z, guards and sentinels, isolation of paths and sequences (post_cases.paths_per_step)."""
    print(post_cases.run_path_case("cpu", case))


def test_paths_per_step_emission_grid_stride(wave_emu_backend):
    """65585 rows: more than the emission's 1024 wavefronts hold, so its grid-stride loop takes a second turn."""
    print(post_cases.run_path_case("cpu", post_cases.POST_EMIT_CASE))


@pytest.mark.parametrize("kind", ["lstm", "switching"])
def test_model_level_matches_impute(wave_emu_backend, kind):
    before = launches(wave_emu_backend)
    post_cases.model_vs_impute("cpu", kind)
    assert launches(wave_emu_backend) > before


def test_model_level_shapes_and_state(wave_emu_backend):
    """Shapes, training mode and parameters left unchanged, injected draws repeat, argument errors."""
    from kvae import noise
    from kvae.train.imputation import sample_imputation_scores
    for kind in ("lstm", "switching"):
        model = post_cases.small_model(kind)
        model.train()
        before = {k: v.clone() for k, v in model.state_dict().items()}
        x = (torch.rand(2, 6, 1, 32, 32) > 0.7).float()
        mask = torch.tensor([[1.0, 1, 0, 0, 1, 1], [1.0, 0, 0, 1, 1, 0]])
        nz = dict(eps_a=torch.randn(12, 2), gumbel=-torch.empty(2, 6, 3).exponential_().log(), post_z=torch.randn(2, 3, 6, 4),
                  post_a=torch.randn(2, 3, 6, 2))
        with noise.inject(**nz):
            out = model.sample_imputations(x, mask, num_samples=3, emission_noise=True)
            again = model.sample_imputations(x, mask, num_samples=3, emission_noise=True)
        assert out["x"].shape == (2, 3, 6, 1, 32, 32) and out["a"].shape == (2, 3, 6, 2) and out["z"].shape == (2, 3, 6, 4)
        assert out["a_vae"].shape == (2, 6, 2) and out["state_probs"].shape == (2, 6, 3) and out["levels"].shape == (2, 6)
        assert all(torch.equal(out[k], again[k]) for k in ("x", "a", "z"))
        assert float((out["z"][:, 0] - out["z"][:, 1]).abs().max()) > 1e-3   # the paths differ
        assert model.training
        after = model.state_dict()
        assert all(torch.equal(before[k], after[k]) for k in before)
        assert model.sample_imputations(x, mask, decode=False)["x"] is None
        sc = sample_imputation_scores(x, out["x"], mask)
        assert all(v.dim() == 0 and bool(torch.isfinite(v)) for v in sc.values())
        assert float(sc["mse_best"]) <= float(((out["x"][:, 0] - x) ** 2 * (1 - mask)[:, :, None, None, None]).sum()
                                              / ((1 - mask).sum() * 1024)) * 2 + 1e-6
    model = post_cases.small_model()
    x = torch.zeros(2, 3, 1, 32, 32)
    ok = torch.ones(2, 3)
    for bad in (dict(num_samples=0), dict(mask=torch.ones(2, 4)), dict(mask=None), dict(u=torch.zeros(2, 4, 4)), dict(u=torch.zeros(2, 3, 3))):
        kw = dict(dict(mask=ok), **bad)
        with pytest.raises(ValueError):
            model.sample_imputations(x, **kw)


def test_sample_imputation_scores():
    from kvae.train.imputation import sample_imputation_scores
    x = torch.zeros(2, 4, 1, 2, 2)
    mask = torch.tensor([[1.0, 0, 0, 1], [1.0, 1, 1, 1]])
    xs = torch.zeros(2, 2, 4, 1, 2, 2)
    xs[0, 0, 1] = 1.0    # sample 0 of sequence 0 is off by 1 on one hidden frame, sample 1 is exact
    xs[:, :, 0] = 9.0    # observed frames do not count
    sc = sample_imputation_scores(x, xs, mask)
    assert abs(float(sc["mse_mean"]) - 0.25 * 4 / 8) < 1e-7      # ensemble mean off by 0.5 on 4 of the 8 hidden pixels
    assert float(sc["mse_best"]) == 0.0
    assert abs(float(sc["std"]) - 0.5 * 4 / 8) < 1e-7
    none = sample_imputation_scores(x, xs, torch.ones(2, 4))
    assert all(float(v) == 0.0 for v in none.values())


def test_c_entry_point_rejects(wave_emu_backend):
    """KVAE_ERR_DIMS for dims out of range, KVAE_ERR_NULL for missing required pointers or eta without its factor,
    KVAE_ERR_ARG for negative strides."""
    from kvae import _native as N
    buf = torch.zeros(8192)
    ptr = buf.data_ptr()
    lv = torch.zeros(16, dtype=torch.int32)

    def prob(**kw):
        pr = N.PsampleProblem()
        pr.B, pr.S, pr.T, pr.n, pr.p = 1, 1, 2, 4, 2
        for k in ("mus_filt", "Sigmas_filt", "mus_pred", "Sigmas_pred", "z_out", "a_out", "ws"):
            setattr(pr, k, ptr)
        pr.levels_out = lv.data_ptr()
        pr.A, pr.C, pr.Q = N.Stack(ptr, 0, 0), N.Stack(ptr, 0, 0), N.Stack(ptr, 0, 0)
        for k, v in kw.items():
            setattr(pr, k, v)
        return pr

    dll = wave_emu_backend.dll
    call = lambda pr: dll.kvae_lgssm_posterior_sample(ctypes.byref(pr), None)
    assert dll.kvae_lgssm_posterior_sample_ws_floats(ctypes.byref(prob())) == 2 * 36
    assert dll.kvae_lgssm_posterior_sample_ws_floats(ctypes.byref(prob(n=17))) == 0
    for kw in (dict(n=0), dict(n=17), dict(p=0), dict(p=17), dict(B=0), dict(S=0), dict(T=0)):
        assert call(prob(**kw)) == 1, kw
    for kw in (dict(mus_filt=None), dict(Sigmas_filt=None), dict(mus_pred=None), dict(Sigmas_pred=None), dict(z_out=None),
               dict(a_out=None), dict(levels_out=None), dict(ws=None), dict(A=N.Stack(None, 0, 0)), dict(C=N.Stack(None, 0, 0)),
               dict(Q=N.Stack(None, 0, 0)), dict(eta=ptr)):
        assert call(prob(**kw)) == 2, kw
    for kw in (dict(A=N.Stack(ptr, -1, 0)), dict(Q=N.Stack(ptr, 0, -4))):
        assert call(prob(**kw)) == 4, kw
    assert call(prob(stages=4)) == 4 and call(prob(stages=-1)) == 4
    assert call(prob(stages=1, z_out=None, a_out=None, C=N.Stack(None, 0, 0))) == 0     # gains alone need no path operands
    assert call(prob(stages=2, mus_filt=None, Sigmas_pred=None, levels_out=None, A=N.Stack(None, 0, 0))) == 0
    assert call(prob(stages=1, levels_out=None)) == 2 and call(prob(stages=2, z_out=None)) == 2
    assert dll.kvae_lgssm_posterior_sample(None, None) == 2
    assert call(prob(eta=ptr, LR=ptr, eps=ptr)) == 0


def test_kernels_have_no_scratch():
    """The resource report of every instantiation of both kernels (gfx950 cross-compile): 0 bytes of scratch per lane."""
    src = ROOT / "kalman-vae_amd" / "csrc" / "kvae_lgssm_post.hip"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-amdgpu-mfma-vgpr-form", "-c",
                        str(src), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S*k_post_\S*)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == 7 and len(scratch) == 7, (names, scratch)
    assert sum("k_post_gains" in n for n in names) == 3 and sum("k_post_paths" in n for n in names) == 3 and sum("k_post_emit" in n for n in names) == 1
    assert all(s == 0 for s in scratch), list(zip(names, scratch))


def test_kernel_bodies_under_sanitizers():
    """A standalone driver of csrc/lgssm_post.h on emulated wavefronts (tests/hostsim/post_asan_driver.cpp), built with
    -fsanitize=address,undefined and run as a child process: n = 4 and n = 16 (and a run-time n), ragged B*T and B*S, T = 1."""
    out = ROOT / "tests" / "hostsim" / "post_asan_driver"
    src = ROOT / "tests" / "hostsim" / "post_asan_driver.cpp"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-fno-sanitize-recover=undefined", "-o", str(out), str(src)], check=True, cwd=ROOT)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(out)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "POST-ASAN-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
