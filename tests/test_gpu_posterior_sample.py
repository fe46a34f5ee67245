"""GPU tier of KalmanFilter.sample_posterior / KVAE.sample_imputations on gfx950: the cases of tests/test_posterior_sample.py on
the device (reference fixtures, moments at S = 8192, restatement, per-item and per-step cases, ladder, model level), a large case against the torch path,
determinism, and training left bit-identical."""
import pytest
import torch

import post_cases

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("name,kind", post_cases.FIXTURES)
def test_noise_free_matches_reference_smoother_gpu(name, kind):
    post_cases.golden_noise_free(name, kind, DEV)


@pytest.mark.parametrize("name,kind", post_cases.FIXTURES)
def test_moments_match_reference_smoother_gpu(name, kind):
    """S = 8192, seed 1, draws from a CPU generator: mean, covariance and lag-one cross-covariance within 5 standard errors of the
    reference smoother's at every (b, t, i, j) (tests/test_posterior_sample.py has the restatement's own figures)."""
    e_mean, e_cov, e_lag = post_cases.golden_moments(name, DEV)
    assert e_mean <= 5 and e_cov <= 5 and e_lag <= 5, (e_mean, e_cov, e_lag)


@pytest.mark.parametrize("n,per_step_Q", [(4, True), (4, False), (16, True), (16, False), (5, True), (5, False)])
def test_kernels_vs_restatement_gpu(n, per_step_Q):
    pr = post_cases.random_problem(n, 2, B=3, S=7, T=9, seed=10 * n + per_step_Q, per_step_Q=per_step_Q)
    post_cases.paths_vs_restatement(DEV, pr, want_levels=[0])


@pytest.mark.parametrize("n,p,B,S,T,kw", [
    (4, 2, 2, 70, 5, {}), (16, 3, 1, 70, 3, {}), (4, 2, 3, 5, 1, {}), (16, 2, 2, 3, 1, {}), (4, 2, 3, 5, 2, {}), (5, 3, 2, 4, 2, {}),
    (4, 2, 5, 1, 6, {}), (16, 2, 2, 1, 4, {}), (4, 2, 3, 4, 6, dict(with_noise=False)), (16, 2, 2, 3, 4, dict(with_noise=False)),
    (4, 2, 3, 4, 6, dict(emission_noise=True)), (16, 5, 2, 3, 4, dict(emission_noise=True)), (7, 16, 2, 3, 4, dict(emission_noise=True)),
])
def test_kernels_shapes_gpu(n, p, B, S, T, kw):
    pr = post_cases.random_problem(n, p, B=B, S=S, T=T, seed=n + p + B + S + T, **kw)
    post_cases.paths_vs_restatement(DEV, pr, want_levels=[0])


@pytest.mark.parametrize("n", [4, 16, 5])
def test_packed_record_is_bit_identical_gpu(n):
    pr = post_cases.random_problem(n, 2, B=3, S=5, T=6, seed=40 + n, emission_noise=True)
    plain = post_cases.run_paths(DEV, pr)
    rec, slots = post_cases.pack_record(pr)
    packed = post_cases.run_paths(DEV, pr, packed=rec.to(DEV), slots=slots)
    for x, y in zip(plain, packed):
        assert torch.equal(x, y)


@pytest.mark.parametrize("n", [4, 16])
def test_misaligned_operands_take_the_fallback_gpu(n):
    pr = post_cases.random_problem(n, 2, B=3, S=5, T=6, seed=50 + n)

    def shift(t):
        buf = torch.empty(t.numel() + 4, device=DEV)   # device allocations are at least 16-byte aligned
        v = buf[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v

    off = dict(pr, **{k: shift(pr[k]) for k in ("eps", "Sigmas_filt", "Sigmas_pred", "A", "Cm", "Q")})
    post_cases.paths_vs_restatement(DEV, pr, got=post_cases.run_paths(DEV, off))


def test_ladder_levels_per_item_gpu():
    post_cases.check_ladder(DEV)
    post_cases.check_ladder(DEV, impl="torch")


@pytest.mark.parametrize("case", post_cases.POST_GAIN_CASES, ids=post_cases.post_case_id)
def test_gains_per_item_gpu(case):
    print(post_cases.run_gain_case(DEV, case))


@pytest.mark.parametrize("name", list(post_cases.LADDER_CASES))
def test_ladder_per_item_gpu(name):
    print(post_cases.ladder_per_item(DEV, name))


@pytest.mark.parametrize("case", post_cases.POST_RING_CASES + post_cases.POST_SHAPE_CASES, ids=post_cases.post_case_id)
def test_paths_per_step_gpu(case):
    print(post_cases.run_path_case(DEV, case))


def test_paths_per_step_emission_grid_stride_gpu():
    print(post_cases.run_path_case(DEV, post_cases.POST_EMIT_CASE))


@pytest.mark.parametrize("kind", ["lstm", "switching"])
def test_model_level_matches_impute_gpu(kind):
    post_cases.model_vs_impute(DEV, kind)


@pytest.mark.parametrize("n", [4, 16])
def test_large_case_matches_torch_path_gpu(n):
    """8192 paths, 16384 items (B = 512, S = 16, T = 32): the kernels against the torch path on the GPU.  Bar as for the
    restatement, with the torch recursion in fp64 in its place: max(1e-4, 4 x the distance of the fp32 torch path from it)."""
    from kvae.kalman import lgssm_ops
    pr = post_cases.random_problem(n, 2, B=512, S=16, T=32, seed=80 + n, emission_noise=True)
    d = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in pr.items()}
    got = lgssm_ops.posterior_paths(impl="kernel", **d)
    f32 = lgssm_ops.posterior_paths(impl="torch", **d)
    f64 = lgssm_ops.posterior_paths_torch(**{k: (v.double() if isinstance(v, torch.Tensor) else v) for k, v in d.items()})
    for name, x, f, r in zip(("z", "a"), got[:2], f32[:2], f64[:2]):
        bar = max(1e-4, 4 * float((f.double() - r).abs().max()))
        err = float((x.double() - r).abs().max())
        print(name, n, "err", err, "bar", bar)
        assert err <= bar, (name, err, bar)
    assert int(got[2].abs().max()) == 0 and torch.equal(got[2], f32[2])


def _noise(B, S, T, n=4, p=2, K=3, seed=3):
    g = torch.Generator().manual_seed(seed)
    return dict(eps_a=torch.randn(B * T, p, generator=g).to(DEV), gumbel=(-torch.empty(B, T, K).exponential_(generator=g).log()).to(DEV),
                post_z=torch.randn(B, S, T, n, generator=g).to(DEV), post_a=torch.randn(B, S, T, p, generator=g).to(DEV))


@pytest.mark.parametrize("kind", ["lstm", "switching"])
def test_determinism_gpu(kind):
    """Same injected noise -> same bits, twice."""
    from kvae import noise
    model = post_cases.small_model(kind).to(DEV)
    x = (torch.rand(3, 9, 1, 32, 32, generator=torch.Generator().manual_seed(2)) > 0.7).float().to(DEV)
    mask = torch.ones(3, 9, device=DEV)
    mask[:, 2:6] = 0
    outs = []
    for _ in range(2):
        with noise.inject(**_noise(3, 4, 9)):
            outs.append(model.sample_imputations(x, mask, num_samples=4, emission_noise=True))
    for k in ("a", "z", "x", "a_vae", "state_probs", "levels"):
        assert torch.equal(outs[0][k], outs[1][k]), k
    assert float((outs[0]["z"][:, 0] - outs[0]["z"][:, 1]).abs().max()) > 1e-3


@pytest.mark.parametrize("kind", ["lstm", "switching"])
def test_training_unaffected_gpu(kind):
    """Trainer(use_graph=True): step -> sample_imputations -> step gives the same bits as two steps, with the same injected noise."""
    from kvae import noise
    from kvae.train.train import Trainer
    B, T = 4, 8
    x = (torch.rand(B, T, 1, 32, 32, generator=torch.Generator().manual_seed(3)) > 0.7).float().to(DEV)
    g = torch.Generator().manual_seed(12)
    nz = dict(eps_a=torch.randn(B * T, 2, generator=g).to(DEV), eps_z=torch.randn(B, T, 4, generator=g).to(DEV),
              gumbel=(-torch.empty(B, T, 3).exponential_(generator=g).log()).to(DEV))
    mask = torch.ones(B, T, device=DEV)
    mask[:, 3:6] = 0

    def run(with_sampling):
        torch.manual_seed(6)
        model = post_cases.small_model(kind).to(DEV)
        tr = Trainer(model, lr=3e-3, grad_clip_norm=10.0, use_graph=True)
        with noise.inject(**nz):
            tr.step(x)
        if with_sampling:
            out = model.sample_imputations(x, mask, num_samples=3)
            assert bool(torch.isfinite(out["x"]).all())
        with noise.inject(**nz):
            out = tr.step(x)
        torch.cuda.synchronize()
        return float(out["loss"]), torch.cat([p.detach().flatten() for p in model.parameters()]).cpu()

    l0, p0 = run(False)
    l0b, p0b = run(False)
    l1, p1 = run(True)
    if l0 == l0b and torch.equal(p0, p0b):   # training repeats bit for bit: so must the run with sampling in between
        assert l1 == l0 and torch.equal(p1, p0)
    else:   # not bitwise repeatable on its own: within the spread of two plain runs
        assert abs(l1 - l0) <= 2 * abs(l0b - l0) and float((p1 - p0).abs().max()) <= 2 * float((p0b - p0).abs().max())
