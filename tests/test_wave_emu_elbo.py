"""CPU tier: the (16,16,2) ELBO kernels of csrc/lgssm_n16_elbo.h - the code `kvae_lgssm_elbo16.hip` wraps in __global__ functions
(probe, zfix, one step per wavefront, four steps per wavefront) - on emulated wavefronts (tests/hostsim/wave_emu.h; their DPP
traffic inside row-group-dependent branches meets on row-scoped rendezvous), checked per (b,t) against a float64 run of the torch
oracle (parity_cases.n16_elbo_per_step).  The launch reports the kernel family it ran (levels[2]), so nothing here can pass on
the generic bodies of the host simulation.  The same kernels go under AddressSanitizer + UBSan in tests/test_hostsim_asan.py."""
import pytest
import torch

import parity_cases
from hostsim.build import build as build_hostsim

torch.set_num_threads(4)
PROBE, MAIN = 4, 5   # indices of kvae_wemu_launches: ELBO probe / main launches at n = 16


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
    return [lib.dll.kvae_wemu_launches(i) for i in (PROBE, MAIN)]


@pytest.mark.parametrize("family", [2, 3])
@pytest.mark.parametrize("grads", [True, False])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("B", [1, 3])
def test_elbo_n16_per_step(wave_emu_backend, family, grads, T, B):
    """Every T % 4 (ragged last four-step group, T = 1 without a Q probe), one and three sequences (one of them masked entirely),
    with and without gradients (both GRADS instantiations of both layouts; per-step Q: HAS_GQ)."""
    before = launches(wave_emu_backend)
    parity_cases.n16_elbo_per_step("cpu", B, T, family, (0, 0), grads)
    after = launches(wave_emu_backend)
    assert after[0] > before[0] and after[1] > before[1], (before, after)   # the emulated kernels are what ran


@pytest.mark.parametrize("family", [2, 3])
@pytest.mark.parametrize("levels", [(0, 0), (0, 1), (3, 0), (5, 0), (2, 5)])
def test_elbo_n16_levels_per_step(wave_emu_backend, family, levels):
    """_safe_cholesky past level 0 (jitter ladder and diagonal fallback, for Sigma_s and for Q; a raised Sigma_s level redoes
    the parked samples in elbo_zfix) at T = 7: a ragged last four-step group."""
    before = launches(wave_emu_backend)
    parity_cases.n16_elbo_per_step("cpu", 2, 7, family, levels, True)
    after = launches(wave_emu_backend)
    assert after[0] > before[0] and after[1] > before[1], (before, after)


@pytest.mark.parametrize("levels", [(0, 0), (0, 1)])
def test_elbo_n16_shared_q_with_its_gradient(wave_emu_backend, levels):
    """A Q shared by the batch whose gradient is wanted stays on one step per wavefront (family 2, HAS_GQ)."""
    parity_cases.n16_elbo_per_step("cpu", 3, 5, 2, levels, True, q_shared=True)


@pytest.mark.parametrize("name,levels", [("jitter_n16_q_level1", [0, 1]), ("jitter_n16_sigma_level2", [2, 0]),
                                         ("jitter_n16_diag_fallback", [0, 5]), ("jitter_n16_sigma_diag_fallback", [5, 0])])
def test_elbo_n16_jitter_goldens(wave_emu_backend, name, levels):
    """The reference's own outputs past level 0 (tests/golden), computed by the emulated kernels (per-step Q_list: family 2)."""
    before = launches(wave_emu_backend)
    parity_cases.jitter_golden("cpu", name, levels, family=2)
    after = launches(wave_emu_backend)
    assert after[0] > before[0] and after[1] > before[1], (before, after)


def test_elbo_n16_unaligned_takes_the_generic_kernels(wave_emu_backend):
    """A Sigma_s stack 4 bytes off a 16-byte boundary fails the gate (family 0) and gives what the aligned call gives."""
    parity_cases.n16_elbo_unaligned("cpu")


def test_xcd_contiguous_is_a_permutation(wave_emu_backend):
    """The workgroup -> (b,t) remap of every ELBO launch hits each unit exactly once, for any grid: all grids up to 4100 and
    the configs[4] shard's B*ceil(T/4) = 25600 and B*T = 102400."""
    f = wave_emu_backend.dll.kvae_wemu_xcd_contiguous_is_permutation
    bad = [nwg for nwg in list(range(1, 4101)) + [25600, 102400] if f(nwg) != 1]
    assert not bad, bad[:20]
