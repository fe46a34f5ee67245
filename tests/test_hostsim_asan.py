"""Run a slice of the host-simulated kernels under AddressSanitizer + UBSan (GPU sanitizers are unavailable on the
pool, so the CPU build of the kernel bodies is the sanitizer target).  Executed in a subprocess with libasan
preloaded; any heap/stack overflow or UB in the bodies aborts it."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]

SCRIPT = r"""
import sys
sys.path[:0] = [%(root)r, %(root)r + "/kalman-vae_amd", %(root)r + "/tests"]
import torch
from kvae import _native
from hostsim.build import build
_native._set_test_backend(_native.LgssmLib(build(sanitize=True)))
import parity_cases
for dims in ((3, 9, 4, 4, 2, 3), (2, 7, 3, 2, 1, 2), (2, 5, 16, 16, 2, 1), (1, 1, 4, 4, 2, 3)):
    parity_cases.vs_oracle_random("cpu", *dims)
parity_cases.safe_cholesky_levels("cpu")
parity_cases.lstm_vs_torch("cpu", 2, 5, 2, 50)
parity_cases.regime_vs_torch("cpu", 2, 6, 3, 0.7, False)
parity_cases.vae_epilogue_vs_torch("cpu", 2, 3, 4, 4, 2, True)
parity_cases.conv_edge_vs_torch("cpu", 2)
parity_cases.enc_mid_vs_torch("cpu", 2, 8)
parity_cases.dec_up_vs_torch("cpu", 2, 4)
parity_cases.vae_heads_vs_torch("cpu", 5)
# the product's wavefront-level kernels (lgssm_m4.h / lgssm_q4.h, lgssm_n16.h) on emulated wavefronts (hostsim/wave_emu.h):
# ragged last wavefront (19 sequences, 16 per wavefront), the tails of the unrolled loops (T = 3, T = 1), 16-byte accesses
# (UBSan's alignment check covers every one of them)
lib = _native.lib_for(torch.zeros(1))
lib.dll.kvae_hostsim_wave_emu(1)
for dims in ((19, 3, 4, 4, 2, 3), (1, 1, 4, 4, 2, 2), (2, 3, 16, 16, 2, 2)):
    parity_cases.vs_oracle_random("cpu", *dims)
lib.dll.kvae_wemu_m4_split_max_b(0)      # (4,4,2) again in its single-launch form (the one batches above 2048 sequences take)
parity_cases.vs_oracle_random("cpu", 19, 4, 4, 4, 2, 3)
lib.dll.kvae_wemu_m4_split_max_b(-1)
assert min(lib.dll.kvae_wemu_launches(i) for i in range(4)) > 0
# the (16,16,2) ELBO kernels (lgssm_n16_elbo.h): per-step Q with its gradient (k_elbo_n16<true, true>), the four-steps-per-
# wavefront layout with a ragged last group (T = 5), the diagonal fallback of Sigma_s (elbo_zfix redoes the samples)
parity_cases.n16_elbo_per_step("cpu", 2, 3, 2, (0, 0), True)
parity_cases.n16_elbo_per_step("cpu", 2, 5, 3, (0, 0), True)
parity_cases.n16_elbo_per_step("cpu", 3, 5, 2, (5, 0), True)
assert min(lib.dll.kvae_wemu_launches(i) for i in (4, 5)) >= 3
# the recurrent kernels on emulated workgroups (hostsim/wave_emu_rnn.cpp; their LDS arrays are heap objects of exactly their size):
# k_lstm_*_fast / k_gru_*_fast read float4 from rows padded from 50 to 52 floats and index c_seq, h_seq and dx one step back or
# ahead (T = 1: no neighbour at all); the lane-grid regime kernels fetch one step ahead from clamped addresses (T = 1, T = 2: the
# last step of the last sequence ends the buffer); thread per sequence with B = 65: a second block with 63 idle lanes
assert lib.dll.kvae_wemu_selftest() == 0
for T in (1, 3):
    parity_cases.lstm_per_step("cpu", 2, T)
    parity_cases.bigru_per_step("cpu", 2, T)
for T, K, hard in ((1, 8, False), (2, 8, True), (2, 3, False), (1, 1, False)):
    parity_cases.regime_per_step("cpu", 2, T, K, 0.7, hard, "grid", tau_dev=hard)
lib.dll.kvae_wemu_regime_grid_max_b(0)
parity_cases.regime_per_step("cpu", 65, 2, 3, 0.7, False, "tpp")
parity_cases.regime_per_step("cpu", 65, 1, 8, 0.7, False, "tpp", tau_dev=True)
lib.dll.kvae_wemu_regime_grid_max_b(-1)
parity_cases.regime_per_step("cpu", 2, 3, 9, 0.7, False, "lds")
assert min(lib.dll.kvae_wemu_rnn_launches(i) for i in range(10)) > 0, [lib.dll.kvae_wemu_rnn_launches(i) for i in range(10)]
lib.dll.kvae_hostsim_wave_emu(0)
print("ASAN-OK")
"""


def test_hostsim_under_asan():
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not asan or not Path(asan).exists():
        pytest.skip("libasan not available")
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1",
               OMP_NUM_THREADS="2")
    r = subprocess.run([sys.executable, "-c", SCRIPT % {"root": str(ROOT)}], env=env, capture_output=True, text=True,
                       timeout=900)
    assert "ASAN-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
