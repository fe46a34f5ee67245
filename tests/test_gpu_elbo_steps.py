"""GPU tier (-m gpu): the ELBO kernels built from csrc/lgssm_elbo.h - k_elbo_probe_tpp / k_elbo_tpp<SDims<4,4,2>> (one thread per
step) and k_elbo_probe<D> / k_elbo<D> (one wavefront per step: SDims<4,4,2>, SDims<16,16,2>, RDims) - one (b,t) at a time against
a float64 run of the torch oracle (parity_cases.elbo_per_step).  Every case asserts the kernel family the launch reports in
levels[2], so none passes on another kernel.  KVAE_ELBO_TPP and KVAE_N16 are read once per process: the lists that need them run
in a fresh child process each."""
import os
import subprocess
import sys

import pytest

import parity_cases

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("case", parity_cases.ELBO_TPP_CASES, ids=parity_cases.elbo_case_id)
def test_elbo_per_step_tpp_gpu(case):
    """Thread-per-step (4,4,2), the default kernel of every (4,4,2) ELBO call: the ragged last block, a block that ends
    mid-sequence, T = 1 and T = 2, the poisoned matrix at q = 0 / 63 / 64 / last."""
    print(parity_cases.run_elbo_case(DEV, "tpp", case, family=1))


@pytest.mark.parametrize("case", parity_cases.ELBO_RT_CASES, ids=parity_cases.elbo_case_id)
def test_elbo_per_step_runtime_dims_gpu(case):
    print(parity_cases.run_elbo_case(DEV, "rt", case, family=0))


@pytest.mark.parametrize("case", parity_cases.ELBO_N16W_CASES, ids=parity_cases.elbo_case_id)
def test_elbo_per_step_n16_wave_gpu(case):
    """(16,16,2) with Sigma_s 4 bytes off a 16-byte boundary: the gate of kvae_lgssm_elbo sends it to k_elbo<SDims<16,16,2>>."""
    print(parity_cases.run_elbo_case(DEV, "n16w", case, family=0))


@pytest.mark.parametrize("fam,env", [("n4w", {"KVAE_ELBO_TPP": "0"}), ("n16w", {"KVAE_N16": "0"})], ids=["n4w_KVAE_ELBO_TPP0", "n16w_KVAE_N160"])
def test_elbo_per_step_switched_gpu(fam, env):
    """The wave-per-step (4,4,2) list under KVAE_ELBO_TPP=0 and the (16,16,2) list under KVAE_N16=0, family 0 asserted per case."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path[:0] = [%r, %r, %r]; import parity_cases as p; p.run_elbo_list('cuda', %r, 0)"
            % (root, os.path.join(root, "kalman-vae_amd"), os.path.join(root, "tests"), fam))
    r = subprocess.run([sys.executable, "-c", code], env={**os.environ, **env}, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stderr[-3000:]
    assert "ELBO_WORST " + fam in r.stdout
