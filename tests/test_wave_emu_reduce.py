"""CPU tier: the kernels that run in every training step of every preset - k_rnn_wgrad_partial<RT> / k_rnn_wgrad_final
(csrc/rnn_wgrad.h: LDS staging, the 16x16x4 MFMA operand layout, the step index carried by adds, clamped loads),
mixw::k_mix_fwd_wave / k_mix_bwd_wave / k_mix_bwd_fold (csrc/mix_wave.h) and the four linear-head kernels (csrc/small_linear.h,
dynamic LDS) - as the product's own __global__ functions on emulated workgroups (tests/hostsim/wave_emu.h, wave_emu_reduce.cpp),
checked one row at a time against float64 torch under the bars of parity_cases.RNN_STEP_TOL.  The launch geometry comes from the
functions the .hip units call (wg_geometry, mix_fwd_geometry / mix_bwd_geometry, sl_rows_per_block); the test-only setters lower
the caps the product passes as constants, so that chunks of several stages, capped slabs and 32 / 64 rows per block run at a few
hundred rows.  Every case asserts from the launch counters which kernel instance ran (or that the gate sent the call to the
element-wise twins).  The cases live in parity_cases and are shared with tests/test_gpu_parity.py; the sanitizer run is a
stand-alone driver (tests/hostsim/reduce_asan_driver.cpp) with every buffer at its exact size."""
import ctypes as C
import os
import subprocess
import threading
from pathlib import Path

import pytest
import torch

import parity_cases
from hostsim.build import build as build_hostsim

torch.set_num_threads(4)
ROOT = Path(__file__).resolve().parents[1]

# names of kvae_wemu_rnn_launches(10 ..): one per kernel instance (wave_emu_reduce.cpp)
MIX_INSTANCES = [(4, 1), (4, 2), (4, 3), (8, 1), (8, 2), (8, 3)]
COUNTERS = ([f"wgrad.partial<{rt}>" for rt in (1, 4, 10, 13, 16)] + ["wgrad.final"] + [f"mix.fwd<{k},{e}>" for k, e in MIX_INSTANCES] +
            [f"mix.bwd<{k},{e}>" for k, e in MIX_INSTANCES] + ["mix.fold", "linear.fwd", "linear.softmax_fwd", "linear.bwd", "linear.softmax_bwd"])
SETTERS = ("kvae_wemu_wgrad_max_chunks", "kvae_wemu_wgrad_fill", "kvae_wemu_mix_fwd_max_slabs", "kvae_wemu_mix_bwd_max_slabs",
           "kvae_wemu_linear_min_blocks")


@pytest.fixture(scope="module", autouse=True)
def wave_emu_backend():
    from kvae import _native
    lib = _native.LgssmLib(build_hostsim())
    _native._set_test_backend(lib)
    lib.dll.kvae_hostsim_wave_emu(1)
    yield lib
    for name in SETTERS:
        getattr(lib.dll, name)(-1)
    lib.dll.kvae_hostsim_wave_emu(0)
    _native._set_test_backend(None)


@pytest.fixture(scope="module", autouse=True)
def sanitizer_run(tmp_path_factory):
    """The build (one compiler process, ~5 s) and the run of the sanitizer driver go on in a thread of their own while the cases
    of this file run, so that the file costs the longer of the two, not the sum; test_kernels_under_sanitizers collects it."""
    out = tmp_path_factory.mktemp("reduce_asan") / "reduce_asan_driver"
    src = ROOT / "tests" / "hostsim" / "reduce_asan_driver.cpp"
    res = {}

    def work():
        try:
            subprocess.run(["g++", "-std=c++17", "-O1", "-g1", "-pthread", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                            "-fno-sanitize-recover=undefined", "-I", str(ROOT / "tests" / "hostsim" / "stub"), "-o", str(out), str(src)],
                           check=True, cwd=ROOT, capture_output=True, text=True)
            env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
            res["run"] = subprocess.run([str(out)], env=env, capture_output=True, text=True, timeout=600)
        except Exception as e:   # reported by the test
            res["error"] = repr(e) + str(getattr(e, "stderr", "") or "")[-4000:]

    res["thread"] = threading.Thread(target=work)
    res["thread"].start()
    yield res
    res["thread"].join()


class Launched:
    """with Launched(lib, {"wgrad.partial<13>": 1, "wgrad.final": 1}): ... - the launches of the block, all of them, by instance."""

    def __init__(self, lib, want):
        self.lib, self.want = lib, {k: v for k, v in want.items() if v}

    def counts(self):
        return [self.lib.dll.kvae_wemu_rnn_launches(10 + i) for i in range(len(COUNTERS))]

    def __enter__(self):
        self.before = self.counts()
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            got = {n: a - b for n, a, b in zip(COUNTERS, self.counts(), self.before) if a != b}
            assert got == self.want, (got, self.want)


class Setting:
    """with Setting(lib, "kvae_wemu_wgrad_max_chunks", 2): ... - a launch-geometry argument lowered for the block."""

    def __init__(self, lib, name, value):
        self.fn, self.value = getattr(lib.dll, name), value

    def __enter__(self):
        self.fn(self.value)

    def __exit__(self, *a):
        self.fn(-1)


def wgrad_launches(batch):
    return {f"wgrad.partial<{parity_cases.wgrad_instance(batch)}>": 1, "wgrad.final": 1}


def mix_launches(K, E, fwd=1, bwd=1):
    inst = parity_cases.mix_instance(K, E)
    if inst is None:
        return {}
    return {"mix.fwd<%d,%d>" % inst: fwd, "mix.bwd<%d,%d>" % inst: bwd, "mix.fold": bwd}


def linear_launches(F, O, softmax):
    want = {"linear.softmax_fwd": 1, "linear.softmax_bwd": 1} if softmax else {"linear.fwd": 1, "linear.bwd": 1}
    want.update(wgrad_launches([(0, 0, F, 0, O, 0)]))   # dW | db: one reduction with R = O rows
    return want


def _ws_floats(lib, batch):
    from kvae import _native as N
    arr = (N.WgradProblem * len(batch))()
    for slot, (Bsz, T, H, I, R, shift) in zip(arr, batch):
        slot.N, slot.R, slot.H, slot.I, slot.bias, slot.T, slot.shift = Bsz * T, R, H, I, 1, T, shift
    return int(lib.dll.kvae_rnn_wgrad_ws_floats(arr, len(batch)))


def _cpad(c):
    return (c[2] + c[3] + 1 + 15) // 16 * 16


# ---- the weight-gradient reduction --------------------------------------------------------------------------------------------
def test_rnn_wgrad_workspace_size(wave_emu_backend):
    """kvae_rnn_wgrad_ws_floats is the kernels' size here - problems x chunk cap x the largest R x Cpad of the batch - and follows
    the cap setter; the plain-loop twin needs no workspace (1 float) with the emulation off."""
    lib = wave_emu_backend
    for batch in parity_cases.WGRAD_BATCH_CASES:
        per = max(c[4] * _cpad(c) for c in batch)
        assert _ws_floats(lib, batch) == per * 256 * len(batch)
        with Setting(lib, "kvae_wemu_wgrad_max_chunks", 3):
            assert _ws_floats(lib, batch) == per * 3 * len(batch)
    lib.dll.kvae_hostsim_wave_emu(0)
    try:
        assert _ws_floats(lib, parity_cases.WGRAD_BATCH_CASES[0]) == 1
    finally:
        lib.dll.kvae_hostsim_wave_emu(1)


@pytest.mark.parametrize("case", parity_cases.WGRAD_ROW_CASES, ids=str)
def test_rnn_wgrad_per_row(wave_emu_backend, case):
    with Launched(wave_emu_backend, wgrad_launches([case])):
        parity_cases.rnn_wgrad_per_row("cpu", *case)


@pytest.mark.parametrize("batch", parity_cases.WGRAD_BATCH_CASES, ids=lambda b: "+".join(str(c[4]) for c in b))
def test_rnn_wgrad_batched(wave_emu_backend, batch):
    """The product's LSTM + head pair, four problems of different R / column groups / N, the ABI limits R = C = 256."""
    with Launched(wave_emu_backend, wgrad_launches(batch)):
        parity_cases.rnn_wgrad_batch_per_row("cpu", batch)


def test_rnn_wgrad_batched_one_chunk(wave_emu_backend):
    """The fill rule: with 8 workgroups to share among 4 problems x 2 column groups every problem is ONE chunk - 70 rows are three
    stages, the 5-row problem a single partial one."""
    batch = parity_cases.WGRAD_BATCH_CASES[1]
    with Setting(wave_emu_backend, "kvae_wemu_wgrad_fill", 8), Launched(wave_emu_backend, wgrad_launches(batch)):
        parity_cases.rnn_wgrad_batch_per_row("cpu", batch)


def test_rnn_wgrad_refusals(wave_emu_backend):
    with Launched(wave_emu_backend, {}):
        parity_cases.rnn_wgrad_refusals("cpu")


@pytest.mark.parametrize("case", parity_cases.WGRAD_STAGE_CASES, ids=str)
def test_rnn_wgrad_stages(wave_emu_backend, case):
    """Chunks of four or five 32-row stages through the chunk cap: the step index advanced by 32 % T per stage, the full-stage
    branch of `fetch`, a partial last stage, chunk starts inside a sequence."""
    *shape, cap = case
    with Setting(wave_emu_backend, "kvae_wemu_wgrad_max_chunks", cap), Launched(wave_emu_backend, wgrad_launches([shape])):
        parity_cases.rnn_wgrad_per_row("cpu", *shape)


def test_rnn_wgrad_stages_at_the_product_cap(wave_emu_backend):
    """8320 rows without any setter: 256 chunks of 36 rows, a full stage and a partial one each, T = 32."""
    case = (260, 32, 13, 3, 5, -1)
    with Launched(wave_emu_backend, wgrad_launches([case])):
        parity_cases.rnn_wgrad_per_row("cpu", *case)


# ---- the mixture ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", parity_cases.MIX_ROW_CASES + parity_cases.MIX_ROW_CASES_EDGE, ids=str)
def test_mix_per_row(wave_emu_backend, case):
    with Launched(wave_emu_backend, mix_launches(*case[2:])):
        parity_cases.mix_per_row("cpu", *case)


@pytest.mark.parametrize("case", parity_cases.MIX_CAPPED_CASES, ids=str)
def test_mix_capped_slabs(wave_emu_backend, case):
    """More than 16 rows per slab, not a multiple of the 4 rows of an RB group, forward and backward (on the card: > 32768 rows)."""
    *shape, fcap, bcap = case
    lib = wave_emu_backend
    with Setting(lib, "kvae_wemu_mix_fwd_max_slabs", fcap), Setting(lib, "kvae_wemu_mix_bwd_max_slabs", bcap), \
            Launched(lib, mix_launches(*shape[2:])):
        parity_cases.mix_per_row("cpu", *shape)


@pytest.mark.parametrize("rows,K,E,misalign", [(21, 3, 768, None), (37, 5, 132, None), (1, 2, 128, None), (21, 3, 768, "partials"),
                                               (21, 3, 768, "g_out"), (21, 3, 48, None)])
def test_mix_accumulate_flag_guarded(wave_emu_backend, rows, K, E, misalign):
    """accumulate_alpha = 1, then 0, through the C ABI in guarded buffers; a misaligned g_out or partials takes the twins."""
    want = {} if misalign else mix_launches(K, E, fwd=0, bwd=2)
    with Launched(wave_emu_backend, want):
        parity_cases.mix_accumulate_guarded("cpu", rows, K, E, misalign)


# ---- the linear heads -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", parity_cases.LINEAR_ROW_CASES + parity_cases.LINEAR_ROW_CASES_EDGE, ids=str)
def test_small_linear_per_row(wave_emu_backend, case):
    with Launched(wave_emu_backend, linear_launches(case[1], case[2], case[3])):
        parity_cases.small_linear_per_row("cpu", *case)


@pytest.mark.parametrize("case", parity_cases.LINEAR_BLOCK_CASES, ids=str)
def test_small_linear_rows_per_block(wave_emu_backend, case):
    """16, 32 and 64 rows per block with a ragged last block, and one block of 64 (sl_stage_rows with u up to 15)."""
    *shape, min_blocks, rows = case
    lib = wave_emu_backend
    n = 1
    for d in shape[0]:
        n *= d
    with Setting(lib, "kvae_wemu_linear_min_blocks", min_blocks), Launched(lib, linear_launches(shape[1], shape[2], shape[3])):
        assert lib.dll.kvae_wemu_linear_rows_per_block(shape[1], shape[2], C.c_int64(n)) == rows
        parity_cases.small_linear_per_row("cpu", *shape)


def test_rows_per_block_of_the_product():
    """The thresholds the GPU tier's large cases rest on: 16 rows below 8192, 32 from there, 64 from 16384 rows on; 16 when W
    leaves no room for more."""
    from kvae import _native
    f = _native.LgssmLib(build_hostsim()).dll.kvae_wemu_linear_rows_per_block
    got = [f(F, O, C.c_int64(n)) for F, O, n in [(17, 5, 8191), (17, 5, 8192), (17, 5, 16383), (17, 5, 16384), (128, 96, 1 << 20)]]
    assert got == [16, 32, 32, 64, 16], got


# ---- the tier itself --------------------------------------------------------------------------------------------------------
def test_off_means_the_plain_twins(wave_emu_backend):
    """With the emulation off the host simulation is what it was: the plain-loop twins, no emulated launch."""
    lib = wave_emu_backend
    lib.dll.kvae_hostsim_wave_emu(0)
    try:
        with Launched(lib, {}):
            parity_cases.rnn_wgrad_per_row("cpu", *parity_cases.WGRAD_ROW_CASES[1])
            parity_cases.mix_per_row("cpu", 5, 9, 3, 768)
            parity_cases.small_linear_per_row("cpu", *parity_cases.LINEAR_ROW_CASES[0])
    finally:
        lib.dll.kvae_hostsim_wave_emu(1)


def test_kernels_under_sanitizers(sanitizer_run):
    """The same kernels in a stand-alone program (tests/hostsim/reduce_asan_driver.cpp) built with -fsanitize=address,undefined and
    run as a child process: the ragged and limit cases above with every input, output, ws and partials buffer a heap block of
    exactly the size the size functions report.  (Built and run beside the cases above: see the fixture.)"""
    sanitizer_run["thread"].join()
    assert "error" not in sanitizer_run, sanitizer_run["error"]
    r = sanitizer_run["run"]
    assert r.returncode == 0 and "REDUCE-ASAN-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
