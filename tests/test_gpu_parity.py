"""GPU tier (-m gpu): the gfx950 library against the goldens captured from the reference, against the
CPU oracle on seeded inputs, and at BASELINE config sizes.  Every call goes through the C ABI of
include/kvae_lgssm.h (ctypes -> libkvae_lgssm.so); nothing here can pass on a CPU fallback because
the product has none (test_native_loaded asserts the HIP library is the one mapped in)."""
import ctypes as C

import pytest
import torch

from golden_util import JITTER_CASES, LATENT_CASES, SMOOTH_KEYS, load, rel_err, stability_state_dict, sub
import parity_cases
from parity_cases import _random_problem
from test_hostsim_ops import check_latent, make_filter, run_latent

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_native_loaded():
    from kvae import _native
    lib = _native.hip_lib()
    assert "gfx950" in lib.build_info
    with open("/proc/self/maps") as f:
        assert "libkvae_lgssm.so" in f.read()
    assert _native._test_backend is None


@pytest.mark.parametrize("name,kind", LATENT_CASES)
def test_latent_gpu(name, kind):
    """smooth + elbo + gradients vs the reference's own outputs (ELBO / smoothed means within 1e-4 rel)."""
    g = load(name)
    kf = make_filter(g, kind, DEV)
    a, outs, elbo = run_latent(kf, g, DEV)
    check_latent(kf, g, a, outs, elbo, name, tol_scale=2.0, kind=kind)


@pytest.mark.parametrize("batch", [1, 4])
def test_rocket_gpu(batch):
    from kvae import noise
    from kvae.kalman.kalman_filter import KalmanFilter
    from kvae.kalman.switch_dyn_param import SwitchingDynamicsParameter
    g = load(f"rocket_B{batch}")
    dyn = SwitchingDynamicsParameter(g["A"], g["B"], g["C"])
    kf = KalmanFilter(2.0, 4.0, g["mu0"], g["Sigma0"], dyn).to(DEV)
    Y, U = g["Y"].to(DEV), g["U"].to(DEV)
    with torch.no_grad(), noise.inject(eps_z=g["eps_z"]):
        outs = kf.smooth(Y, U)
        elbo = kf.elbo(outs[0], outs[1], Y, U, outs[6], outs[7], outs[8])
    for k, v in zip(SMOOTH_KEYS, outs):
        assert rel_err(v.cpu(), g[k]) < 5e-5, k
    assert rel_err(elbo.cpu(), g["elbo"]) < 5e-5


@pytest.mark.parametrize("name,kind,K", [("stability_lstm", "lstm", 3), ("stability_switching", "switching", 3),
                                         ("stability_lstm_K7_T100", "lstm", 7),
                                         ("stability_switching_K7_T100", "switching", 7)])
def test_stability_recipe_gpu(name, kind, K):
    """The reference's tests/test_imputation_stability.py recipe through the drop-in KVAE.impute."""
    from kvae import noise
    from kvae.model.model import KVAE
    from kvae.utils.config import KVAEConfig
    g = load(name)
    T = int(g["T"])
    model = KVAE(KVAEConfig(dynamics_model=kind, num_modes=K))
    model.load_state_dict(stability_state_dict(kind, K), strict=True)
    model.to(DEV).eval()
    torch.manual_seed(123)
    x = torch.randn(2, T, 1, 32, 32).to(DEV)
    with noise.inject(eps_a=g["eps_a"], gumbel=g.get("gumbel")):
        out = model.impute(x, g["mask"].to(DEV))
    sl = slice(None) if g["x_recon"].shape[1] == T else slice(None, None, 10)
    for k in ("x_recon", "x_imputed", "x_filtered"):
        assert (out[k].cpu()[:, sl] - g[k]).abs().max() < 2e-6, k
    for k in ("a_imputed", "a_filtered"):
        assert (out[k].cpu() - g[k]).abs().max() < 1e-6, k


@pytest.mark.parametrize("name,kind", [("trainstep_lstm_K3", "lstm"), ("trainstep_switch_K3", "switching")])
def test_train_step_gpu(name, kind):
    """One full step (forward, loss, backward, clip, Adam) vs the reference's recorded step."""
    from kvae import noise
    from kvae.model.model import KVAE
    from kvae.utils.config import KVAEConfig
    g = load(name)
    model = KVAE(KVAEConfig(dynamics_model=kind, num_modes=3))
    model.load_state_dict(sub(g, "sd."), strict=True)
    model.to(DEV).train()
    model.beta = float(g["beta"])
    x = g["frames"].float().to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=float(g["lr"]))
    with noise.inject(eps_a=g["eps_a"], eps_z=g["eps_z"], gumbel=g.get("gumbel")):
        out = model(x, mask=torch.ones(x.shape[:2], device=DEV))
        losses = model.compute_loss(x, out, mask=torch.ones(x.shape[:2], device=DEV))
    losses["loss"].backward()
    gn = torch.nn.utils.clip_grad_norm_(model.parameters(), float(g["clip"]))
    opt.step()
    assert rel_err(losses["loss"].detach().cpu(), g["loss"]) < 1e-4
    assert rel_err(losses["elbo_kf"].detach().cpu(), g["elbo_kf"]) < 1e-4
    assert rel_err(out["mus_smooth"].detach().cpu(), g["mus_smooth"]) < 1e-4
    assert rel_err(gn.cpu(), g["grad_norm"]) < 1e-3
    for k, p in model.named_parameters():
        ref = float(g["gradnorm." + k])
        assert abs(float(p.grad.norm()) - ref) <= 2e-3 * ref + 1e-6, k
        if "grad." + k in g and ref > 1e-6:
            assert rel_err(p.grad.cpu(), g["grad." + k]) < 2e-3, k


@pytest.mark.parametrize("B,T,n,m,p,K", [(256, 50, 4, 4, 2, 3), (7, 33, 4, 4, 2, 3), (5, 17, 3, 2, 1, 2),
                                         (3, 9, 8, 5, 3, 4), (64, 200, 16, 16, 2, 3), (1, 1, 4, 4, 2, 3),
                                         (2, 2, 16, 16, 2, 1), (512, 200, 16, 16, 2, 3), (8, 200, 16, 16, 2, 3),
                                         (5, 1, 16, 16, 2, 2), (8192, 6, 4, 4, 2, 3), (3, 2, 4, 4, 2, 3), (17, 3, 4, 4, 2, 2),
                                         (2, 3, 16, 16, 2, 2)])
def test_vs_oracle_random(B, T, n, m, p, K):
    """Values vs the C oracle at every size, incl. the FULL BASELINE configs[4] shard (512, 200, 16); gradients vs the
    torch oracle's autograd up to configs[1] size (256, 50, 4) and for n = 16 at (8, 200, 16).  (8192, 6, 4): many wavefronts of the sixteen-
    sequences-per-wavefront n = 4 kernels, with a ragged last one in (7, 33, 4).  T = 1, 2, 3: the tails of the sweeps' unrolled
    loops (two operand sets at n = 4, three at n = 16, rotated by name)."""
    parity_cases.vs_oracle_random(DEV, B, T, n, m, p, K)


@pytest.mark.parametrize("B,T,n", [(3, 10, 16), (2, 7, 16), (5, 9, 4)])
def test_vs_oracle_dense_shared_q(B, T, n):
    """A full SPD process noise, T not a multiple of four: the four-steps-per-wavefront ELBO of the (16,16,2) kernels (ragged last
    wavefront, chol(Q)^-1 and its transpose) and the n = 4 kernels, values and gradients."""
    parity_cases.vs_oracle_random(DEV, B, T, n, n, 2, 2, dense_q=True)


@pytest.mark.parametrize("B,T,K", [(17, 5, 1), (3, 10, 1), (4, 5, 1), (17, 12, 1), (17, 5, 3)])
def test_single_mode_n16_vs_fp64_oracle(B, T, K):
    """K = 1 at n = 16: the float32 torch tape is itself ~1e-2 from float64 there (found by a random sweep over shapes), so the
    gradients are held to the float64 oracle instead; (17, 5, 3) shows the same sweep point is well conditioned with three modes."""
    tape = parity_cases.grads_vs_fp64_oracle(DEV, B, T, 16, K)
    if K == 3:
        assert tape < 3e-3


@pytest.mark.parametrize("B,T,K", [(8, 200, 3), (3, 37, 1)])
def test_values_n16_vs_fp64_oracle(B, T, K):
    """Smoothed means / covariances / ELBO at n = 16 within max(1e-4, 4 x the float32 oracle's own distance from float64) of the
    float64 oracle: north_star's 1e-4 wherever float32 can deliver it, and an explicit, measured budget where it cannot (a
    single mode, K = 1, is the ill-conditioned corner round 2's sweep found: float32 itself is 1e-2 off there)."""
    report = parity_cases.values_vs_fp64_oracle(DEV, B, T, 16, K)
    if K > 1:
        assert all(mine < 2e-3 for mine, _ in report.values()), report


def test_backward_at_the_full_shard_equals_its_slices():
    """k_smooth_bwd_n16 at the full configs[4] shard (512, 200, 16) against the same kernel on 64 independent 8-sequence slices
    (the size gradient parity with the torch oracle is checked at): sequences do not interact, so every gradient of the big
    launch must be BIT-identical to the slice launches' - a wavefront-indexing or hand-off-record bug at 512 wavefronts shows here."""
    parity_cases.backward_shard_vs_slices(DEV, 512, 200, 16, 8)


def test_dec_up_workgroup_cap():
    parity_cases.dec_up_workgroup_cap(DEV)


def test_colsum_pair():
    parity_cases.colsum_pair_vs_torch(DEV)


def test_n16_generic_fallback():
    parity_cases.n16_generic_fallback(DEV)


def test_n4_generic_fallback():
    parity_cases.n4_generic_fallback(DEV)


def test_n16_indefinite_q_takes_the_pivoted_solve():
    parity_cases.n16_indefinite_q(DEV)


def test_linearity_full_size():
    parity_cases.linearity(DEV, 256, 50)


@pytest.mark.parametrize("n,B,T", [(4, 2, 4), (16, 2, 4), (16, 40, 10)])
def test_safe_cholesky_levels(n, B, T):
    parity_cases.safe_cholesky_levels(DEV, n, B, T)


@pytest.mark.parametrize("n,B,T", [(16, 5, 10), (16, 33, 7), (4, 3, 6), (7, 2, 5)])
def test_safe_cholesky_levels_shared_q(n, B, T):
    """Raised levels and the diagonal fallback with a batch-wide Q, for Sigma_s and Q: at n = 16 on the matrix-core kernels of
    BOTH layouts (the launch reports its family), no generic backup launch."""
    parity_cases.safe_cholesky_levels_shared_q(DEV, n, B, T)


@pytest.mark.parametrize("family", [2, 3])
@pytest.mark.parametrize("grads", [True, False])
@pytest.mark.parametrize("B,T", [(1, 1), (1, 2), (1, 3), (1, 4), (1, 5), (3, 1), (3, 2), (3, 3), (3, 4), (3, 5), (7, 9), (33, 13)])
def test_elbo_n16_per_step_gpu(family, grads, B, T):
    """The (16,16,2) ELBO kernels per (b,t) against float64 (parity_cases.n16_elbo_per_step): every T % 4, and grids that are
    not multiples of the 8 XCDs and span more than one round of the XCD remap ((7,9), (33,13))."""
    parity_cases.n16_elbo_per_step(DEV, B, T, family, (0, 0), grads)


@pytest.mark.parametrize("family", [2, 3])
@pytest.mark.parametrize("levels", [(0, 0), (0, 1), (3, 0), (5, 0), (2, 5)])
def test_elbo_n16_levels_per_step_gpu(family, levels):
    parity_cases.n16_elbo_per_step(DEV, 2, 7, family, levels, True)


@pytest.mark.parametrize("levels", [(0, 0), (0, 1)])
def test_elbo_n16_shared_q_with_its_gradient_gpu(levels):
    parity_cases.n16_elbo_per_step(DEV, 3, 5, 2, levels, True, q_shared=True)


def test_elbo_n16_configs4_slice_per_step_gpu():
    """A configs[4]-shaped slice (T = 200, shared Q, gradients): four steps per wavefront, per (b,t)."""
    parity_cases.n16_elbo_per_step(DEV, 8, 200, 3, (0, 0), True)


def test_elbo_n16_unaligned_takes_the_generic_kernels_gpu():
    parity_cases.n16_elbo_unaligned(DEV)


@pytest.mark.parametrize("name,levels", JITTER_CASES)
def test_jitter_golden_gpu(name, levels):
    """_safe_cholesky past level 0, pinned to the REFERENCE (fixtures driven through its own elbo)."""
    parity_cases.jitter_golden(DEV, name, levels)


def test_c_abi_direct_and_errors():
    """Call the C ABI with raw device pointers (what a non-Python host would do) and check the error codes."""
    from kvae import _native as N
    lib = N.hip_lib()
    B, T, n, m, p = 3, 5, 4, 4, 2
    A, Bm, Cm, alpha, Y, U, mask, eps = _random_problem(B, T, n, m, p, 1, 3, DEV)
    R, Q = 0.03 * torch.eye(p, device=DEV), 0.02 * torch.eye(n, device=DEV)
    mu0, S0 = torch.zeros(n, device=DEV), 20.0 * torch.eye(n, device=DEV)
    prob = N.Problem()
    prob.B, prob.T, prob.n, prob.m, prob.p = B, T, n, m, p
    prob.A, prob.Bm = N.Stack(A.data_ptr(), 0, 0), N.Stack(Bm.data_ptr(), 0, 0)
    prob.C, prob.Q = N.Stack(Cm.data_ptr(), 0, 0), N.Stack(Q.data_ptr(), 0, 0)
    prob.R, prob.mu0, prob.Sigma0, prob.Y, prob.U = R.data_ptr(), mu0.data_ptr(), S0.data_ptr(), Y.data_ptr(), U.data_ptr()
    outs = [torch.empty(B, T, n, device=DEV) if i % 2 == 0 else torch.empty(B, T, n, n, device=DEV) for i in range(6)]
    st = N.States(*[o.data_ptr() for o in outs], None)
    assert lib.dll.kvae_lgssm_smooth_fwd(C.byref(prob), C.byref(st), None) == 0
    torch.cuda.synchronize()
    from oracle import c_oracle
    c = lambda t: t.cpu()
    ref = c_oracle.smooth(c(Y), c(U), None, c(A[0]), c(Bm[0]), c(Cm[0]), c(Q), c(R), c(mu0), c(S0))
    assert rel_err(outs[4].cpu(), ref["mus_smooth"]) < 1e-4
    prob.n = 17
    assert lib.dll.kvae_lgssm_smooth_fwd(C.byref(prob), C.byref(st), None) == 1      # KVAE_ERR_DIMS
    prob.n = n
    prob.Y = None
    assert lib.dll.kvae_lgssm_smooth_fwd(C.byref(prob), C.byref(st), None) == 2      # KVAE_ERR_NULL
    assert lib.dll.kvae_mix_fwd(None, None, None, 1, 1, 1, None) == 2
    assert lib.dll.kvae_mix_fwd(N.ptr(alpha), N.ptr(A), N.ptr(outs[1]), 1, 17, 1, None) == 4   # KVAE_ERR_ARG


@pytest.mark.parametrize("B,T,I,H", [(256, 50, 2, 50), (3, 7, 2, 50), (2, 5, 5, 13)])
def test_lstm_gpu(B, T, I, H):
    parity_cases.lstm_vs_torch(DEV, B, T, I, H)


@pytest.mark.parametrize("N,C,H,W,r,relu", [(64, 32, 8, 8, 2, True), (7, 1, 16, 16, 2, False), (33, 32, 16, 16, 1, True)])
def test_vae_epilogue_gpu(N, C, H, W, r, relu):
    parity_cases.vae_epilogue_vs_torch(DEV, N, C, H, W, r, relu)


@pytest.mark.parametrize("B,T,K,tau,hard", [(256, 50, 3, 1.0, False), (4, 100, 7, 0.5, False), (3, 10, 3, 0.7, True),
                                            (32, 100, 7, 0.7, True), (5, 9, 8, 1.3, False), (2, 1, 2, 0.5, False), (3, 4, 9, 1.0, False)])
def test_regime_gpu(B, T, K, tau, hard):
    parity_cases.regime_vs_torch(DEV, B, T, K, tau, hard)


@pytest.mark.parametrize("B,T", [(256, 50), (3, 7), (2, 1)])
def test_bigru_gpu(B, T):
    """kvae_bigru_fwd/bwd vs torch.nn.GRU(bidirectional) on the CPU: values and every gradient."""
    from kvae.kalman.lgssm_ops import BiGruSequence
    torch.manual_seed(B + T)
    ref = torch.nn.GRU(2, 50, batch_first=True, bidirectional=True)
    x = torch.randn(B, T, 2)
    wgt = torch.randn(B, T, 100)
    xr = x.clone().requires_grad_(True)
    (ref(xr)[0] * wgt).sum().backward()
    names = ["weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0", "weight_ih_l0_reverse", "weight_hh_l0_reverse",
             "bias_ih_l0_reverse", "bias_hh_l0_reverse"]
    params = [getattr(ref, n).detach().clone().to(DEV).requires_grad_(True) for n in names]
    xd = x.clone().to(DEV).requires_grad_(True)
    h = BiGruSequence.apply(xd, *params)
    (h * wgt.to(DEV)).sum().backward()
    assert rel_err(h.detach().cpu(), ref(x)[0].detach()) < 2e-5
    assert rel_err(xd.grad.cpu(), xr.grad) < 2e-4
    for n, got in zip(names, params):
        assert rel_err(got.grad.cpu(), getattr(ref, n).grad) < 2e-4, n


RNN_STEP_SHAPES = [(256, 50, "all"), (256, 50, "first"), (256, 50, "last"), (3, 7, "all"), (1, 1, "all"), (3, 2, "last"),
                   (1, 3, "first")]


@pytest.mark.parametrize("B,T,steps", RNN_STEP_SHAPES)
def test_lstm_per_step_gpu(B, T, steps):
    """k_lstm_fwd_fast / k_lstm_bwd_fast against float64 nn.LSTM, one (b,t) slice at a time (h, gates, c_seq, dx)."""
    print(parity_cases.lstm_per_step(DEV, B, T, steps))


@pytest.mark.parametrize("B,T,steps", RNN_STEP_SHAPES)
def test_bigru_per_step_gpu(B, T, steps):
    """k_gru_fwd_fast / k_gru_bwd_fast against float64 nn.GRU(bidirectional), one (b,t) slice at a time (h, dx)."""
    print(parity_cases.bigru_per_step(DEV, B, T, steps))


# (B, T, K, tau, hard, tau_dev): the large cases of test_regime_gpu, the edges (T = 1, K = 1, K = 8, K > 8: LDS bodies), and
# B = 4097: one sequence above the lane-grid kernels' batch threshold, which the default dispatch hands to a thread per sequence
REGIME_STEP_CASES = [(256, 50, 3, 1.0, False, False), (32, 100, 7, 0.7, True, False), (4, 100, 7, 0.5, False, True),
                     (5, 9, 8, 1.3, False, True), (2, 1, 2, 0.5, False, False), (3, 4, 9, 1.0, False, False),
                     (3, 7, 16, 0.7, False, True), (3, 10, 3, 0.7, True, False), (3, 5, 1, 0.7, False, False),
                     (4097, 3, 3, 0.7, False, False), (4097, 2, 7, 1.3, False, True)]


@pytest.mark.parametrize("B,T,K,tau,hard,tau_dev", REGIME_STEP_CASES)
def test_regime_per_step_gpu(B, T, K, tau, hard, tau_dev):
    print(parity_cases.regime_per_step(DEV, B, T, K, tau, hard, None, tau_dev))


@pytest.mark.parametrize("B,T,K,tau,hard", [(4097, 3, 3, 0.7, False), (4097, 2, 7, 1.3, False)])
def test_regime_gpu_above_the_grid_threshold(B, T, K, tau, hard):
    """More than 4096 sequences: the thread-per-sequence kernels k_regime_{fwd,bwd}_tpp<K> (64 sequences per block, a ragged
    last block with one lane in use)."""
    parity_cases.regime_vs_torch(DEV, B, T, K, tau, hard)


@pytest.mark.parametrize("mode", ["0", "1", "2"])
def test_regime_switch_selects_working_kernels(mode):
    """KVAE_REGIME_TPP (read once per process) chooses the family of the regime chain: 1 (default) the lane-grid kernels up to
    4096 sequences and a thread per sequence above, 2 a thread per sequence always (every instance K = 2..8, at B = 65: a ragged
    second block), 0 the LDS bodies.  The GPU build has no launch counter, so each mode runs the per-step cases in a fresh
    process of its own, each against float64: whatever family the switch selects has to pass them."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path[:0] = [%r, %r, %r]; import parity_cases as p\n"
            "for K in range(1, 9):\n"
            "    p.regime_per_step('cuda', 65, 3, K, 0.7, False, None, K %% 2 == 0)\n"
            "for c in %r:\n"
            "    p.regime_per_step('cuda', *c)\n"
            % (root, os.path.join(root, "kalman-vae_amd"), os.path.join(root, "tests"),
               [c[:5] + (None, c[5]) for c in REGIME_STEP_CASES]))
    r = subprocess.run([sys.executable, "-c", code], env={**os.environ, "KVAE_REGIME_TPP": mode}, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]


@pytest.mark.parametrize("N", [1, 37, 1000, 2000])
def test_conv_edge_gpu(N):
    """Direct decoder-head / encoder-stem kernels vs torch conv2d; 1000 / 2000 frames exercise the frame-strided weight-gradient loop."""
    parity_cases.conv_edge_vs_torch(DEV, N)


@pytest.mark.parametrize("N", [1, 37, 12800])
def test_vae_heads_gpu(N):
    """Fused encoder heads + reparameterisation, decoder fc, latent regulariser vs torch."""
    parity_cases.vae_heads_vs_torch(DEV, N)


@pytest.mark.parametrize("N,side", [(1, 8), (2, 8), (7, 8), (1031, 8), (1, 4), (8, 4), (13, 4), (4099, 4)])
def test_dec_up_gpu(N, side):
    """Register-stationary MFMA decoder blocks vs torch (ragged last iteration, more iterations than workgroups)."""
    parity_cases.dec_up_vs_torch(DEV, N, side)


@pytest.mark.parametrize("which,side", [("enc_mid", 8), ("dec_up", 4)])
def test_conv_chunked_launches_gpu(which, side, monkeypatch):
    """20000 frames = two launches (CHUNK = 16384).  They must equal ONE launch over all frames and five independent
    4000-frame calls (a size the kernels are checked at against the CPU above): outputs and data gradients bit-identical,
    weight gradients to fp32 summation order.  The external reference at this size is the nine-tap float64 restatement on
    sampled frames (conv_layer_per_frame, also test_vae_conv_chunk_boundary_gpu): torch's CPU convolution backward (fp32 and
    fp64 disagree with each other above 16384 frames) and MIOpen's Winograd data gradient (8e-3 off) both proved unreliable here."""
    from kvae.vae.fused import DecoderUp, EncoderMid
    print(parity_cases.conv_layer_per_frame(DEV, which, 20000, side))
    Fn = EncoderMid if which == "enc_mid" else DecoderUp
    N, co = 20000, (32 if which == "enc_mid" else 128)
    g = torch.Generator().manual_seed(7)
    x = torch.relu(torch.randn(N, 32, side, side, generator=g)).to(DEV)
    W = (0.08 * torch.randn(co, 32, 3, 3, generator=g)).to(DEV)
    b = (0.1 * torch.randn(co, generator=g)).to(DEV)
    o_side = side // 2 if which == "enc_mid" else 2 * side
    up = torch.linspace(-1, 1, N * 32 * o_side * o_side, device=DEV).view(N, 32, o_side, o_side)

    def run(slices):
        Ws, bs = W.clone().requires_grad_(True), b.clone().requires_grad_(True)
        outs, gxs = [], []
        for lo, hi in slices:
            xs = x[lo:hi].clone().requires_grad_(True)
            out = Fn.apply(xs, Ws, bs)
            (out * up[lo:hi]).sum().backward()
            outs.append(out.detach())
            gxs.append(xs.grad)
        return torch.cat(outs), torch.cat(gxs), Ws.grad, bs.grad
    chunked = run([(0, N)])
    pieces = run([(i, i + 4000) for i in range(0, N, 4000)])
    monkeypatch.setattr(Fn, "CHUNK", 1 << 30)
    single = run([(0, N)])
    for other in (single, pieces):
        assert torch.equal(chunked[0], other[0]) and torch.equal(chunked[1], other[1])
        for a, r in zip(chunked[2:], other[2:]):
            assert rel_err(a.cpu(), r.cpu()) < 1e-4   # fp32 summation order over 3e5 cancelling terms


@pytest.mark.parametrize("N,side", [(1, 16), (2, 16), (7, 16), (1031, 16), (1, 8), (8, 8), (13, 8), (4099, 8)])
def test_enc_mid_gpu(N, side):
    """MFMA stride-2 encoder layers vs torch; odd frame counts exercise the ragged last iteration, the large ones the
    persistent loop (more iterations than workgroups)."""
    parity_cases.enc_mid_vs_torch(DEV, N, side)


def test_mix_gpu():
    """Mixture-of-K step records on the streaming kernels (one pass over the gradient records) vs torch.einsum autograd."""
    parity_cases.mix_vs_torch(DEV)


def test_rnn_wgrad_gpu():
    """No library GEMM on the path: LSTM / bi-GRU / head parameter gradients on the f32 matrix cores vs torch products."""
    parity_cases.rnn_wgrad_vs_torch(DEV)


@pytest.mark.parametrize("Bsz,T,H,I,R,shift", parity_cases.WGRAD_ROW_CASES + parity_cases.WGRAD_ROW_CASES_LARGE)
def test_rnn_wgrad_per_row_gpu(Bsz, T, H, I, R, shift):
    """Every k_rnn_wgrad_partial<RT> instance with a ragged last row tile, ragged columns and rows, h_{t-1} / h_{t+1} at the
    sequence boundaries (T = 1: all of them), one output row at a time against float64."""
    print(parity_cases.rnn_wgrad_per_row(DEV, Bsz, T, H, I, R, shift))


@pytest.mark.parametrize("batch", parity_cases.WGRAD_BATCH_CASES, ids=lambda b: "+".join(str(c[4]) for c in b))
def test_rnn_wgrad_batched_gpu(batch):
    """Several problems in one pair of launches: the product's LSTM + head pair (the K-row head under k_rnn_wgrad_partial<13>), four
    problems of different R, column groups and N, the ABI limits R = C = 256; the refusals one past each limit."""
    print(parity_cases.rnn_wgrad_batch_per_row(DEV, batch))


def test_rnn_wgrad_refusals_gpu():
    parity_cases.rnn_wgrad_refusals(DEV)


@pytest.mark.parametrize("Bsz,T,K,E", parity_cases.MIX_ROW_CASES + parity_cases.MIX_ROW_CASES_EDGE + parity_cases.MIX_ROW_CASES_LARGE)
def test_mix_per_row_gpu(Bsz, T, K, E):
    """The streaming mixture kernels (and their element-wise fallback) one (b,t) row at a time against float64: ragged row
    counts, K below the instance's KMAX."""
    print(parity_cases.mix_per_row(DEV, Bsz, T, K, E))


@pytest.mark.parametrize("rows,K,E,misalign", [(21, 3, 768, None), (37, 5, 132, None), (21, 3, 768, "partials")])
def test_mix_accumulate_flag_guarded_gpu(rows, K, E, misalign):
    """accumulate_alpha through the C ABI with every buffer between guard records; a misaligned partials buffer takes the
    element-wise kernels."""
    print(parity_cases.mix_accumulate_guarded(DEV, rows, K, E, misalign))


@pytest.mark.parametrize("lead,F,O,softmax,strided", parity_cases.LINEAR_ROW_CASES + parity_cases.LINEAR_ROW_CASES_LARGE + parity_cases.LINEAR_ROW_CASES_EDGE)   # (appended: the ids count)
def test_small_linear_per_row_gpu(lead, F, O, softmax, strided):
    """The four small_linear.h kernels one row at a time against float64 (contiguous rows and the strided rows of h_seq[:, 0])."""
    print(parity_cases.small_linear_per_row(DEV, lead, F, O, softmax, strided))


def test_small_linear_gpu():
    parity_cases.small_linear_vs_torch(DEV)


@pytest.mark.parametrize("shape", [(256, 50, 1, 32, 32), (2, 3, 1, 32, 32), (1, 2, 3, 5, 7)])
def test_bce_frames_gpu(shape):
    parity_cases.bce_frames_vs_torch(DEV, *shape)


@pytest.mark.parametrize("K,T,n", [(3, 20, 4), (7, 60, 4), (2, 12, 16)])
def test_alpha_lstm_masked_matches_stepwise(K, T, n):
    """Masked frames with the lstm alpha-net: the in-kernel path (network inside the filter kernel, coupled adjoint in
    ONE backward launch) against the product's per-step differentiable path (T nn.LSTM cell steps + T single-step filter
    launches, autograd through all of it) - values, alpha, and every gradient.  The goldens masked_lstm_* pin the same
    path to the reference itself (test_latent_gpu)."""
    from kvae.kalman.lgssm_ops import LgssmSmooth, Slots
    from kvae.model.model import KVAE
    from kvae.utils.config import KVAEConfig
    torch.manual_seed(K)
    model = KVAE(KVAEConfig(dynamics_model="lstm", num_modes=K, z_dim=n))
    with torch.no_grad():
        model.kalman_filter.dyn_params.A.add_(0.05 * torch.randn_like(model.kalman_filter.dyn_params.A))
        model.kalman_filter.dyn_params.head_w.bias.zero_()
        model.kalman_filter.dyn_params.head_w.weight.mul_(3.0)
    kf = model.kalman_filter.to(DEV).train()
    dyn = kf.dyn_params
    B = 5
    a = torch.randn(B, T, 2, device=DEV)
    u = 0.3 * torch.randn(B, T, n, device=DEV)
    mask = (torch.rand(B, T, device=DEV) > 0.4).float()
    mask[:, :3] = 1.0
    w_ms, w_Ss = torch.randn(B, T, n, 1, device=DEV), torch.randn(B, T, n, n, device=DEV)
    w_mf = torch.randn(B, T, n, 1, device=DEV)
    params = list(dyn.parameters())

    def loss_of(outs):
        ms, Ss, mf = outs[0], outs[1], outs[2]
        A_l, C_l = outs[6], outs[8]
        return (ms * w_ms).sum() + (Ss * w_Ss).sum() + (mf * w_mf).sum() + 0.1 * (A_l ** 2).sum() + 0.1 * (C_l ** 2).sum()

    a_f = a.clone().requires_grad_(True)
    dyn.reset_state()
    fast = kf.smooth(a_f, u, mask=mask)                       # in-kernel alpha-network
    alpha_fast = dyn.state_seq.detach().clone()
    g_fast = torch.autograd.grad(loss_of(fast), [a_f] + params, allow_unused=True)

    a_s = a.clone().requires_grad_(True)
    dyn.reset_state()
    mf, Sf, mp, Sp, A_l, B_l, C_l = kf._filter_stepwise(a_s, u, mask)     # reference-shaped per-step path
    ms, Ss, mf2, Sf2, mp2, Sp2 = LgssmSmooth.apply(a_s, u, mask, None, A_l, B_l, C_l, kf.Q, kf.R, kf.mu0, kf.Sigma0, Slots(), True)
    slow = (ms.unsqueeze(-1), Ss, mf2.unsqueeze(-1), Sf2, mp2.unsqueeze(-1), Sp2, A_l, B_l, C_l)
    alpha_slow = dyn.state_seq.detach()
    g_slow = torch.autograd.grad(loss_of(slow), [a_s] + params, allow_unused=True)

    assert rel_err(alpha_fast.cpu(), alpha_slow.cpu()) < 2e-4
    for f_, s_ in zip(fast, slow):
        assert rel_err(f_.detach().cpu(), s_.detach().cpu()) < 5e-4
    names = ["a"] + [k for k, _ in dyn.named_parameters()]
    for name, gf, gs in zip(names, g_fast, g_slow):
        assert (gf is None) == (gs is None), name
        if gf is not None:
            assert rel_err(gf.cpu(), gs.cpu()) < 3e-3, name


def test_explicit_ones_mask_equals_no_mask():
    """The reference's loop passes mask = ones (train.py:41): with lstm dynamics that takes the in-kernel alpha-network
    (no host-side inspection of the mask) and must reproduce the precomputed-alpha path of mask=None."""
    from kvae.model.model import KVAE
    from kvae.utils.config import KVAEConfig
    torch.manual_seed(0)
    model = KVAE(KVAEConfig(dynamics_model="lstm", num_modes=3))
    with torch.no_grad():
        model.kalman_filter.dyn_params.A.add_(0.05 * torch.randn_like(model.kalman_filter.dyn_params.A))
        model.kalman_filter.dyn_params.head_w.bias.zero_()
    kf = model.kalman_filter.to(DEV).train()
    a = torch.randn(6, 15, 2, device=DEV)
    u = torch.zeros(6, 15, 4, device=DEV)
    outs = []
    for mk in (None, torch.ones(6, 15, device=DEV)):
        ar = a.clone().requires_grad_(True)
        kf.dyn_params.reset_state()
        o = kf.smooth(ar, u, mask=mk)
        g = torch.autograd.grad(o[0].sum() + (o[1] ** 2).sum(), [ar] + list(kf.dyn_params.parameters()), allow_unused=True)
        outs.append((o, g))
    for x, y in zip(outs[0][0], outs[1][0]):
        assert rel_err(y.detach().cpu(), x.detach().cpu()) < 2e-4
    for x, y in zip(outs[0][1], outs[1][1]):
        if x is not None:
            assert rel_err(y.cpu(), x.cpu()) < 2e-3


@pytest.mark.parametrize("env", [{"KVAE_WINO": "0"}, {"KVAE_Q4": "0"}, {"KVAE_N16": "0"}, {"KVAE_M4_SPLIT_MAX_B": "0"}])
def test_ab_switches_select_working_kernels(env):
    """The fault-isolation switches that remain (read once per process: direct instead of Winograd decoder blocks, one wavefront
    per sequence at n = 4, run-time-dimension kernels at n = 16 - each also the product's path for operands the specialised
    kernels cannot take) must select kernels that still pass parity: a fresh process per switch."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path[:0] = [%r, %r, %r]; import parity_cases as p; "
            "p.dec_up_vs_torch('cuda', 7, 8); p.dec_up_vs_torch('cuda', 13, 4); "
            "p.vs_oracle_random('cuda', 3, 10, 16, 16, 2, 2, dense_q=True); p.vs_oracle_random('cuda', 19, 11, 4, 4, 2, 3)"
            % (root, os.path.join(root, "kalman-vae_amd"), os.path.join(root, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env={**os.environ, **env}, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]


def test_m4_split_and_single_launch_forms_give_the_same_bits():
    """(4,4,2) below 2048 sequences: chain sweeps + per-step items (3 / 4 launches) against the single-launch form
    (KVAE_M4_SPLIT_MAX_B=0) on the same inputs, a fresh process each (the switch is read once): all six stacks and every gradient
    bit for bit - per-step Q, a mask, upstream gradients on all stacks."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, hashlib; sys.path[:0] = [%r, %r, %r]; import torch, parity_cases as p\n"
            "from kvae.kalman.lgssm_ops import LgssmSmooth, Slots, mix_dynamics\n"
            "B, T, n, K = 37, 23, 4, 3\n"
            "A, Bm, Cm, alpha, Y, U, mask, _ = p._random_problem(B, T, n, n, 2, K, 4242, 'cuda')\n"
            "g = torch.Generator().manual_seed(9)\n"
            "qq = 0.05 * torch.randn(K, n, n, generator=g)\n"
            "Qk = (0.02 * torch.eye(n).repeat(K, 1, 1) + qq @ qq.mT).cuda()\n"
            "R, mu0, S0 = 0.03 * torch.eye(2).cuda(), (0.1 * torch.randn(n, generator=g)).cuda(), 2.0 * torch.eye(n).cuda()\n"
            "w = [(torch.randn(B, T, n, generator=g) if i %% 2 == 0 else torch.randn(B, T, n, n, generator=g)).cuda() for i in range(6)]\n"
            "leaves = [t.clone().requires_grad_(True) for t in (A, Bm, Qk, alpha, Y, U)]\n"
            "rec, offs, _ = mix_dynamics(leaves[3], leaves[:3])\n"
            "outs = LgssmSmooth.apply(leaves[4], leaves[5], mask, rec, None, None, Cm[0], None, R, mu0, S0, "
            "Slots(A=offs[0], B=offs[1], Q=offs[2]), True)\n"
            "sum((o * wi).sum() for o, wi in zip(outs, w)).backward()\n"
            "h = hashlib.sha256()\n"
            "[h.update(t.detach().cpu().numpy().tobytes()) for t in list(outs) + [l.grad for l in leaves]]\n"
            "print('DIGEST', h.hexdigest())\n" % (root, os.path.join(root, "kalman-vae_amd"), os.path.join(root, "tests")))
    digests = []
    for env in ({}, {"KVAE_M4_SPLIT_MAX_B": "0"}):
        r = subprocess.run([sys.executable, "-c", code], env={**os.environ, **env}, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        digests.append([l for l in r.stdout.splitlines() if l.startswith("DIGEST")][-1])
    assert digests[0] == digests[1]


# ---- frame-VAE kernels per (frame, channel) plane / per row against float64 (parity_cases.conv_layer_per_frame and friends) ----
@pytest.mark.parametrize("layer,side", parity_cases.VAE_LAYER_SIDES)
def test_vae_conv_every_residue_gpu(layer, side):
    """N = 1 ... 17: every residue of the frames per iteration / column set of every kernel of the layer, all frames compared."""
    for N in parity_cases.VAE_RESIDUE_N:
        print(N, parity_cases.conv_layer_per_frame(DEV, layer, N, side))


@pytest.mark.parametrize("layer,side,N", parity_cases.VAE_GRID_CASES)
def test_vae_conv_persistent_grid_gpu(layer, side, N):
    """255, 256, 257 and 513 iterations / column sets on 256 persistent workgroups (the last one ragged); 1023 ... 2049 frames on
    the 1024 weight-gradient rows of the edge kernels."""
    print(parity_cases.conv_layer_per_frame(DEV, layer, N, side))


@pytest.mark.parametrize("N", parity_cases.VAE_CHUNK_N)
@pytest.mark.parametrize("layer,side", parity_cases.VAE_LAYER_SIDES)
def test_vae_conv_chunk_boundary_gpu(layer, side, N):
    """One frame short of a launch of CHUNK frames, exactly one, one frame into the second, and 20000: sampled frames against
    float64, the upstream gradient on them alone."""
    print(parity_cases.conv_layer_per_frame(DEV, layer, N, side))


@pytest.mark.parametrize("layer,side", parity_cases.VAE_LAYER_SIDES)
def test_vae_conv_c5_size_gpu(layer, side):
    """512 x 200 frames, what bench.py --config c5 pushes through every layer: seven launches of the chunked ones, 102400
    workgroups over tensors past 2^31 bytes in the edge kernels."""
    print(parity_cases.conv_layer_per_frame(DEV, layer, parity_cases.VAE_C5_N, side))
    torch.cuda.empty_cache()


def _largest_launch(layer, side):
    """The largest N with (N + 2048) x bytes per frame of the launch's largest tensor < 2^31 (kvae_vae.hip)."""
    per_frame = 32 * side * side * 4 if layer == "enc_mid" else 128 * side * side * 4
    return (1 << 31) // per_frame - 2048 - 1


@pytest.mark.parametrize("layer,side", [("enc_mid", 16), ("enc_mid", 8), ("dec_up", 8), ("dec_up", 4)])
def test_vae_conv_largest_single_launch_gpu(layer, side, monkeypatch):
    """CHUNK out of the way: the largest frame count one launch accepts (63487 frames of 32 KiB, 260095 of 8 KiB), where the
    32-bit byte offsets inside a launch come closest to wrapping."""
    N = _largest_launch(layer, side)
    assert N == {32768: 63487, 8192: 260095}[(32 if layer == "enc_mid" else 128) * side * side * 4]
    monkeypatch.setattr(parity_cases._vae_fn(layer), "CHUNK", 1 << 30)
    print(N, parity_cases.conv_layer_per_frame(DEV, layer, N, side))
    torch.cuda.empty_cache()


@pytest.mark.parametrize("layer,side", [("enc_mid", 16), ("dec_up", 8)])
def test_vae_conv_one_frame_more_is_refused_gpu(layer, side):
    """One frame above that through the raw C ABI: KVAE_ERR_ARG from the forward and the backward call, and not a byte of the
    sentinel-filled outputs written.  Every tensor really holds N frames, so a wrong check could not leave its allocations."""
    from kvae import _native as N_
    lib = N_.hip_lib()
    N = _largest_launch(layer, side) + 1
    co, so = (32, side // 2) if layer == "enc_mid" else (128, 2 * side)
    x = torch.zeros(N, 32, side, side, device=DEV)
    W, b = torch.zeros(co, 32, 3, 3, device=DEV), torch.zeros(co, device=DEV)
    out = torch.full((N, 32, so, so), 7.5, device=DEV)
    g_x = torch.full((N, 32, side, side), 7.5, device=DEV)
    pre = "kvae_" + layer
    rows = getattr(lib.dll, pre + "_partial_rows")(N, side)
    wp, bp = torch.full((rows, W.numel()), 7.5, device=DEV), torch.full((rows, co), 7.5, device=DEV)
    st = N_.stream_for(x)
    assert getattr(lib.dll, pre + "_fwd")(N_.ptr(x), N_.ptr(W), N_.ptr(b), N_.ptr(out), N, 32, side, st) == 4      # KVAE_ERR_ARG
    g = torch.zeros_like(out)
    assert getattr(lib.dll, pre + "_bwd")(N_.ptr(x), N_.ptr(W), N_.ptr(g), N_.ptr(g), N_.ptr(g_x), N_.ptr(wp), N_.ptr(bp), N, 32, side,
                                          st) == 4
    torch.cuda.synchronize()
    for t in (out, g_x, wp, bp):
        assert bool((t == 7.5).all())
    assert getattr(lib.dll, pre + "_fwd")(N_.ptr(x), N_.ptr(W), N_.ptr(b), N_.ptr(out), N - 1, 32, side, st) == 0    # ... and N - 1 is taken
    torch.cuda.synchronize()
    assert bool((out[:N - 1] == 0).all()) and bool((out[N - 1] == 7.5).all())


@pytest.mark.parametrize("layer,side", parity_cases.VAE_LAYER_SIDES)
def test_vae_conv_probes_gpu(layer, side):
    """Impulse upstream gradient / impulse input at corners, edges and an interior pixel, in the first and last frame of an
    iteration / column set and of a ragged one: exact zeros outside the receptive field, act(bias) exactly in every other frame."""
    worst = {}
    for kind, frame, pos in parity_cases.vae_probe_cases(layer, side):
        for k, v in parity_cases.conv_probe(DEV, layer, side, kind, frame, pos).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(worst)


@pytest.mark.parametrize("layer,side,N", parity_cases.VAE_SCALE_CASES)
def test_vae_conv_frame_scales_gpu(layer, side, N):
    """Neighbouring frames scaled by 1e-3, 1 and 1e+2: an error of one frame cannot hide behind another frame's size."""
    print(parity_cases.conv_layer_per_frame(DEV, layer, N, side, scales=True))


@pytest.mark.parametrize("layer,side", [("enc_mid", 16), ("enc_mid", 8), ("dec_up", 8), ("dec_up", 4), ("dec_head", 16)])
def test_vae_conv_without_input_gradient_gpu(layer, side):
    parity_cases.conv_no_input_grad(DEV, layer, 13, side)


@pytest.mark.parametrize("N", parity_cases.VAE_HEADS_N + (parity_cases.VAE_C5_N,))
def test_vae_heads_per_row_gpu(N):
    print(parity_cases.vae_heads_per_row(DEV, N))


@pytest.mark.parametrize("B,T", parity_cases.VAE_BCE_CASES + [(512, 200)])
def test_bce_frames_per_row_gpu(B, T):
    print(parity_cases.bce_frames_per_row(DEV, B, T))


@pytest.mark.parametrize("env,which", [({"KVAE_WINO": "0"}, "dec_up"), ({"KVAE_STEM_MFMA": "0"}, "stem"), ({"KVAE_STEM_MFMA": "2"}, "stem")])
def test_vae_variant_kernels_per_frame(env, which):
    """The kernels behind the switches (read once per process), each in a fresh process of its own: the direct decoder blocks
    k_dec_up_*<8|4> (KVAE_WINO=0), the VALU stem weight gradient k_enc_stem_wrw (KVAE_STEM_MFMA=0) and the MFMA one with the mask
    taken from `out` (k_enc_stem_wrw_mfma<false>, =2) through the residue sweep, the grids, the probes, the frame scales and one
    16385-frame case, at the bars of the default kernels."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path[:0] = [%r, %r, %r]; import parity_cases as p; p.vae_variant_cases('cuda', %r)"
            % (root, os.path.join(root, "kalman-vae_amd"), os.path.join(root, "tests"), which))
    r = subprocess.run([sys.executable, "-c", code], env={**os.environ, **env}, capture_output=True, text=True, timeout=900)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stderr[-2000:]


# ---- the sweeps and the coupled alpha-network kernels one (b,t) slice at a time against float64 ----
def _fresh_process(call, env):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path[:0] = [%r, %r, %r]; import parity_cases as p; %s"
            % (root, os.path.join(root, "kalman-vae_amd"), os.path.join(root, "tests"), call))
    r = subprocess.run([sys.executable, "-c", code], env={**os.environ, **env}, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stderr[-2000:]


@pytest.mark.parametrize("case", parity_cases.LGSSM_N4_CASES + parity_cases.LGSSM_N4_ISOLATION_CASES[:6], ids=parity_cases.lgssm_case_id)
def test_lgssm_sweeps_per_step_n4_gpu(case):
    """(4,4,2), every operand on a 16-byte boundary, B <= 2048: k_smooth_fwd_m4 and k_smooth_bwd_m4 in the split form (chain sweeps
    + k_rts_bwd_items_m4), sixteen sequences per wavefront, B = 15 / 17 / 33 with a ragged last wavefront; up="filter" runs
    k_smooth_fwd_m4 forward and k_smooth_bwd_n4 backward (with_rts = 0).  only_b: the upstream gradient on one sequence."""
    print(parity_cases.run_lgssm_case(DEV, case, (4, 4, 2)))


def test_lgssm_sweeps_per_step_n4_single_launch_natural_size_gpu():
    """B = 2049, one sequence above the split: the single-launch k_smooth_fwd_m4 / k_smooth_bwd_m4 at their natural size (129
    wavefronts, the last with one sequence), packed A|B|Q, upstream gradients on all six stacks, per-sequence priors."""
    print(parity_cases.run_lgssm_case(DEV, parity_cases.LGSSM_N4_LARGE_CASE, (4, 4, 2)))


def test_lgssm_sweeps_per_step_n4_single_launch_fresh_process_gpu():
    """The single-launch form below the split (KVAE_M4_SPLIT_MAX_B=0 is read once per process): B = 16, 17, 33, T = 1 ... 5, 24."""
    _fresh_process("p.lgssm_single_launch_cases('cuda')", {"KVAE_M4_SPLIT_MAX_B": "0"})


@pytest.mark.parametrize("case", parity_cases.LGSSM_N4_ODD_CASES, ids=parity_cases.lgssm_case_id)
def test_lgssm_sweeps_per_step_n4_misaligned_gpu(case):
    """(4,4,2) with the packed record / the A stack 4 bytes off a 16-byte boundary: k_smooth_fwd_n4 / k_smooth_bwd_n4."""
    print(parity_cases.run_lgssm_case(DEV, case, (4, 4, 2)))


@pytest.mark.parametrize("case", parity_cases.LGSSM_N16_CASES, ids=parity_cases.lgssm_case_id)
def test_lgssm_sweeps_per_step_n16_gpu(case):
    """(16,16,2), aligned: k_smooth_fwd_n16 / k_smooth_bwd_n16 on the matrix cores (up="filter": k_smooth_fwd_n16 forward, the
    run-time-dimension k_smooth_bwd<D> backward)."""
    print(parity_cases.run_lgssm_case(DEV, case, (16, 16, 2)))


@pytest.mark.parametrize("case", parity_cases.LGSSM_N16_ODD_CASES, ids=parity_cases.lgssm_case_id)
def test_lgssm_sweeps_per_step_n16_misaligned_gpu(case):
    """(16,16,2) with one operand 4 bytes off a 16-byte boundary: k_smooth_fwd_wide (256 threads) and k_smooth_bwd<D>."""
    print(parity_cases.run_lgssm_case(DEV, case, (16, 16, 2)))


@pytest.mark.parametrize("case", parity_cases.LGSSM_RT_CASES, ids=parity_cases.lgssm_case_id)
def test_lgssm_sweeps_per_step_runtime_dims_gpu(case):
    """(2,1,1), (5,3,2), (8,8,3): k_smooth_fwd<D> / k_smooth_bwd<D>, one wavefront per sequence; (12,12,2), (16,8,2): n > 8 takes
    k_smooth_fwd_wide."""
    print(parity_cases.run_lgssm_case(DEV, case))


@pytest.mark.parametrize("B,T,n,m,K,mask_kind,steps,with_rts", parity_cases.ALPHA_LSTM_CASES)
def test_alpha_lstm_per_step_gpu(B, T, n, m, K, mask_kind, steps, with_rts):
    """k_filter_alpha_lstm / k_alpha_lstm_bwd per (b,t) against a float64 run of O.lgssm_smooth(kind="lstm"): (n, m) = (4, 4) the
    SDims<4,4,2> instance, (5, 3) and (16, 16) RDims; t = 0 hidden (the cell's next input is C_0 mu_0|-1), the last step hidden
    (no feedback leaves the sequence), a whole sequence hidden (the feedback chain runs T deep)."""
    print(parity_cases.alpha_lstm_per_step(DEV, B, T, n, m, K, mask_kind, steps, with_rts))
