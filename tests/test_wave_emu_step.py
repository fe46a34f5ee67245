"""CPU tier: the small kernels BETWEEN the compute kernels of every training step - k_grad_sumsq / k_clip_adam (csrc/clip_adam.h),
k_loss_head_fwd / bwd (csrc/vae_heads.h), k_colsum_v4 / k_colsum_v4_pair / k_colsum (csrc/colsum.h), k_emission_means
(csrc/emission_means.h) and the five conv-epilogue kernels (csrc/vae_epilogue.h) - as the product's own __global__ functions on
emulated workgroups (tests/hostsim/wave_emu.h, wave_emu_step.cpp): the cases of tests/step_cases.py that take `lib`, the ones
tests/test_gpu_step_kernels.py runs on the gfx950 library, under the same bars (step_cases.TOL).  The path gates, grids and LDS
sizes come from the functions the .hip units call; test-only setters lower the caps the product passes as constants, so that the
grid-stride rounds (epi_grid's 8192 blocks, the 512 partials and 2048 blocks of clip + Adam) and the chunk edges of the bias kernel
run at a few thousand elements.  Every case asserts from the launch counters which kernel instance ran.  The sanitizer runs are a
stand-alone driver (tests/hostsim/step_asan_driver.cpp), built once with AddressSanitizer + UBSan and once with ThreadSanitizer,
with every buffer ending where its heap block ends."""
import os
import subprocess
import threading
from pathlib import Path

import pytest
import torch

import step_cases as cases
from hostsim.build import build as build_hostsim

torch.set_num_threads(4)
ROOT = Path(__file__).resolve().parents[1]
DEV = "cpu"

# names of kvae_wemu_rnn_launches(33 ..): one per kernel instance (wave_emu_step.cpp)
COUNTERS = ["adam.sumsq", "adam.clip", "head.fwd", "head.bwd", "colsum.v4", "colsum.v4_pair", "colsum", "emission",
            "epi.fwd_v4<1>", "epi.fwd_v4<2>", "epi.fwd", "epi.bwd_bias", "epi.bwd"]
FIRST_COUNTER = 33
# setter -> the product's constant it stands for
SETTERS = {"kvae_wemu_epi_max_blocks": 8192, "kvae_wemu_epi_samples_per_chunk": 32, "kvae_wemu_clip_adam_parts": 512,
           "kvae_wemu_clip_adam_max_blocks": 2048}
SANITIZERS = {"asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"],
              "tsan": ["-fsanitize=thread"]}


@pytest.fixture(scope="module", autouse=True)
def wave_emu_backend():
    from kvae import _native
    lib = _native.LgssmLib(build_hostsim())
    _native._set_test_backend(lib)
    lib.dll.kvae_hostsim_wave_emu(1)
    yield lib
    lib.dll.kvae_hostsim_wave_emu(0)
    _native._set_test_backend(None)


@pytest.fixture(autouse=True)
def product_caps(wave_emu_backend):
    yield
    for name in SETTERS:
        getattr(wave_emu_backend.dll, name)(-1)


@pytest.fixture(scope="module", autouse=True)
def sanitizer_runs(tmp_path_factory):
    """The two builds (one compiler process each) and runs of the sanitizer driver go on in threads of their own while the cases of
    this file run, so that the file costs the longest of them, not the sum; test_kernels_under_sanitizers collects them."""
    src = ROOT / "tests" / "hostsim" / "step_asan_driver.cpp"
    res = {}

    def work(tag):
        out = tmp_path_factory.mktemp("step_" + tag) / ("step_driver_" + tag)
        try:
            subprocess.run(["g++", "-std=c++17", "-O1", "-g1", "-pthread", *SANITIZERS[tag], "-I", str(ROOT / "tests" / "hostsim" / "stub"),
                            "-o", str(out), str(src)], check=True, cwd=ROOT, capture_output=True, text=True)
            env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1",
                       TSAN_OPTIONS="halt_on_error=0:exitcode=66")
            res[tag] = subprocess.run([str(out)], env=env, capture_output=True, text=True, timeout=600)
        except Exception as e:   # reported by the test
            res[tag + "-error"] = repr(e) + str(getattr(e, "stderr", "") or "")[-4000:]

    threads = {tag: threading.Thread(target=work, args=(tag,)) for tag in SANITIZERS}
    for t in threads.values():
        t.start()
    res["threads"] = threads
    yield res
    for t in threads.values():
        t.join()


class Launched:
    """with Launched(lib, {"colsum.v4": 1}): ... - the launches of the block, all of them, by kernel instance."""

    def __init__(self, lib, want):
        self.lib, self.want = lib, {k: v for k, v in want.items() if v}
        assert set(self.want) <= set(COUNTERS), self.want

    def counts(self):
        return [self.lib.dll.kvae_wemu_rnn_launches(FIRST_COUNTER + i) for i in range(len(COUNTERS))]

    def __enter__(self):
        self.before = self.counts()
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            got = {n: a - b for n, a, b in zip(COUNTERS, self.counts(), self.before) if a != b}
            assert got == self.want, (got, self.want)


class Setting:
    """with Setting(lib, "kvae_wemu_epi_max_blocks", 3): ... - a launch-geometry argument lowered for the block."""

    def __init__(self, lib, name, value):
        self.fn, self.value = getattr(lib.dll, name), value

    def __enter__(self):
        self.fn(self.value)

    def __exit__(self, *a):
        self.fn(-1)


# ---- clip + Adam ----------------------------------------------------------------------------------------------------------------
# The two cases that take a second round of both grid-stride loops on the card (512 partials, 2048 blocks) take them here with the
# caps at 2 partials and 3 blocks: 1536 = two full rounds of 3 x 256, 1793 = the same plus a ragged 257; k_grad_sumsq walks both in
# rounds of 2 x 256, and k_clip_adam folds the 2 partials it left.
ADAM_CAPS = (2, 3)
ADAM_LOWERED = {"stride-524288": dict(id="stride-1536-capped", sizes=[1536], seg=False, seed=11),
                "stride-524545": dict(id="stride-1793-capped", sizes=[1793], seg=False, state="random", steps0=[3], seed=12)}


def _adam(lib, id_, fn, launches):
    """Run fn(case) for the case of that id - the lowered stand-in with the caps set, if it has one."""
    c = ADAM_LOWERED.get(id_)
    if c is None:
        with Launched(lib, {"adam.sumsq": launches, "adam.clip": launches}):
            return fn(cases.adam_case_by_id(id_))
    with Setting(lib, "kvae_wemu_clip_adam_parts", ADAM_CAPS[0]), Setting(lib, "kvae_wemu_clip_adam_max_blocks", ADAM_CAPS[1]), \
            Launched(lib, {"adam.sumsq": launches, "adam.clip": launches}):
        return fn(c)


@pytest.mark.parametrize("case", cases.ADAM_IDS)
def test_clip_adam_per_element(wave_emu_backend, case):
    steps = len({**cases.ADAM_SPEC, **cases.adam_case_by_id(case)}["active"])
    _adam(wave_emu_backend, case, lambda c: cases.adam_case(wave_emu_backend, DEV, c), steps)


def test_clip_adam_rejects(wave_emu_backend):
    with Launched(wave_emu_backend, {}):
        cases.adam_rejects(wave_emu_backend, DEV)


@pytest.mark.parametrize("case", ["stride-524545", "layout-block-edges"])
def test_clip_adam_repeatable(wave_emu_backend, case):
    _adam(wave_emu_backend, case, lambda c: cases.adam_repeatable(wave_emu_backend, DEV, c), 2)


def test_clip_adam_nan_gradient(wave_emu_backend):
    with Launched(wave_emu_backend, {"adam.sumsq": 1, "adam.clip": 1}):
        cases.adam_nan_gradient(wave_emu_backend, DEV)


def test_clip_adam_one_partial_for_both_launches(wave_emu_backend):
    """The cap at ONE partial: k_grad_sumsq is a single workgroup walking 2049 elements in nine rounds and writes ws[0] alone; the
    other two floats of the case's workspace keep their sentinel, which a k_clip_adam that folded its own count would add to the
    norm.  Both launches take `parts` from the one ca_parts() call, as the product's entry point does."""
    lib = wave_emu_backend
    with Setting(lib, "kvae_wemu_clip_adam_parts", 1), Launched(lib, {"adam.sumsq": 1, "adam.clip": 1}):
        cases.adam_case(lib, DEV, dict(id="one-partial", sizes=[2049], seg=False, state="random", steps0=[2], seed=13))


# ---- loss head ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.HEAD_IDS)
def test_loss_head_c_abi(wave_emu_backend, case):
    with Launched(wave_emu_backend, {"head.fwd": 1, "head.bwd": 1}):
        cases.head_case(wave_emu_backend, DEV, cases.HEAD_CASES[cases.HEAD_IDS.index(case)])


def test_loss_head_bwd_grid_stride(wave_emu_backend):
    """On the card n = 8192 x 256 + 3; here epi_grid's cap is 3 blocks and n = 2 x 768 + 259: two full rounds and a ragged third."""
    lib = wave_emu_backend
    with Setting(lib, "kvae_wemu_epi_max_blocks", 3), Launched(lib, {"head.bwd": 1}):
        cases.head_bwd_large(lib, DEV, n=2 * 768 + 259)


# ---- column sums ----------------------------------------------------------------------------------------------------------------
def _colsum_kernel(cols, off_in, off_out):
    """The gate of csrc/colsum.h, restated: whole quads of columns and both operands on a 16-byte boundary."""
    return "colsum.v4" if cols % 4 == 0 and off_in == 0 and off_out == 0 else "colsum"


@pytest.mark.parametrize("cols", cases.COLSUM_COLS)
def test_colsum_c_abi(wave_emu_backend, cols):
    want = {}
    for _ in cases.COLSUM_ROWS:
        for oi, oo in cases.COLSUM_PLACES.values():
            k = _colsum_kernel(cols, oi, oo)
            want[k] = want.get(k, 0) + 1
    with Launched(wave_emu_backend, want):
        cases.colsum_abi(wave_emu_backend, DEV, cols)


def test_colsum2_c_abi(wave_emu_backend):
    """The pair kernel when both jobs pass the gate, two single launches otherwise, none for the refused calls."""
    want = {}
    for ra, ca, rb, cb in cases.COLSUM2_CASES:
        for off in (0, 1):
            ka, kb = _colsum_kernel(ca, 0, 0), _colsum_kernel(cb, 0, off)
            for k in (["colsum.v4_pair"] if ka == kb == "colsum.v4" else [ka, kb]):
                want[k] = want.get(k, 0) + 1
    assert want["colsum.v4_pair"] == 2 and want["colsum.v4"] >= 4 and want["colsum"] >= 4
    with Launched(wave_emu_backend, want):
        cases.colsum2_abi(wave_emu_backend, DEV)


# ---- emission means ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,n,p", cases.EMISSION_SHAPES)
def test_emission_means_c_abi(wave_emu_backend, B, T, n, p):
    with Launched(wave_emu_backend, {"emission": 3}):
        cases.emission_abi(wave_emu_backend, DEV, B, T, n, p)


def test_emission_means_rejects(wave_emu_backend):
    with Launched(wave_emu_backend, {"emission": 1}):   # the one valid call the case starts with
        cases.emission_rejects(wave_emu_backend, DEV)


# ---- conv epilogues ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,off_in,off_out,kernel", cases.EPI_FWD_CASES, ids=cases.case_id)
def test_epilogue_fwd_per_element(wave_emu_backend, shape, off_in, off_out, kernel):
    with Launched(wave_emu_backend, {kernel: 2}):   # relu off and on
        cases.epi_fwd_case(wave_emu_backend, DEV, shape, off_in, off_out)


@pytest.mark.parametrize("shape,kernel", cases.EPI_STRIDE_EMU, ids=cases.case_id)
def test_epilogue_fwd_grid_stride(wave_emu_backend, shape, kernel):
    """epi_grid capped at 3 blocks: 1800 quads (or elements) are two full rounds of 768 and a third of 264."""
    lib = wave_emu_backend
    with Setting(lib, "kvae_wemu_epi_max_blocks", 3), Launched(lib, {kernel: 2}):
        cases.epi_fwd_case(lib, DEV, shape)


@pytest.mark.parametrize("shape,relu,want_bias,off", cases.EPI_BWD_CASES, ids=cases.case_id)
def test_epilogue_bwd_per_element(wave_emu_backend, shape, relu, want_bias, off):
    with Launched(wave_emu_backend, {"epi.bwd_bias" if want_bias else "epi.bwd": 2}):   # the call and its repeat
        cases.epi_bwd_case(wave_emu_backend, DEV, shape, relu, want_bias, off)


@pytest.mark.parametrize("N", [1, 3, 4, 5])
def test_epilogue_bwd_chunks_of_two(wave_emu_backend, N):
    """Two samples per chunk: kvae_bias_partial_rows follows the setter, and N = 3, 4, 5 are the chunk edges again."""
    lib = wave_emu_backend
    with Setting(lib, "kvae_wemu_epi_samples_per_chunk", 2), Launched(lib, {"epi.bwd_bias": 2}):
        assert lib.dll.kvae_bias_partial_rows(N) == (N + 1) // 2
        cases.epi_bwd_case(lib, DEV, (N, 3, 2, 2, 2), 1, True, per_chunk=2)
    assert lib.dll.kvae_bias_partial_rows(65) == 3


def test_epilogue_bwd_grid_stride(wave_emu_backend):
    lib = wave_emu_backend
    with Setting(lib, "kvae_wemu_epi_max_blocks", 3), Launched(lib, {"epi.bwd": 2}):
        cases.epi_bwd_case(lib, DEV, cases.EPI_BWD_STRIDE_EMU, 1, False)


def test_epilogue_rejects(wave_emu_backend):
    with Launched(wave_emu_backend, {"epi.bwd_bias": 1}):   # the one valid call the case ends with
        cases.epi_rejects(wave_emu_backend, DEV)


# ---- the tier itself --------------------------------------------------------------------------------------------------------------
def test_setters_hold_the_product_constants(wave_emu_backend):
    """A setter returns the value it replaces: without a test's setting that is the constant kvae_vae.hip passes."""
    for name, constant in SETTERS.items():
        fn = getattr(wave_emu_backend.dll, name)
        assert fn(7) == constant and fn(-1) == 7 and fn(-1) == constant, name


def test_off_means_the_plain_twins(wave_emu_backend):
    """With the emulation off the host simulation is what it was: the plain-loop twins, no emulated launch."""
    lib = wave_emu_backend
    lib.dll.kvae_hostsim_wave_emu(0)
    try:
        with Launched(lib, {}):
            cases.adam_case(lib, DEV, cases.adam_case_by_id("layout-7-300-41"))
            cases.head_case(lib, DEV, cases.HEAD_CASES[0])
            cases.colsum_abi(lib, DEV, 4)
            cases.emission_abi(lib, DEV, *cases.EMISSION_SHAPES[1])
            cases.epi_fwd_case(lib, DEV, *cases.EPI_FWD_CASES[1][:3])
            cases.epi_bwd_case(lib, DEV, *cases.EPI_BWD_CASES[3])
    finally:
        lib.dll.kvae_hostsim_wave_emu(1)


@pytest.mark.parametrize("tag", list(SANITIZERS))
def test_kernels_under_sanitizers(sanitizer_runs, tag):
    """The same kernels in a stand-alone program (tests/hostsim/step_asan_driver.cpp) run as a child process: with
    -fsanitize=address,undefined every operand ends where its heap block ends and every LDS array has its exact size; with
    -fsanitize=thread the lanes' LDS traffic is checked against the barriers, the float atomics of the bias bins being the only
    unordered accesses.  (Built and run beside the cases above: see the fixture.)"""
    sanitizer_runs["threads"][tag].join()
    assert tag + "-error" not in sanitizer_runs, sanitizer_runs.get(tag + "-error")
    r = sanitizer_runs[tag]
    assert r.returncode == 0 and "STEP-SAN-OK" in r.stdout and "Sanitizer" not in r.stderr, r.stdout[-2000:] + r.stderr[-6000:]
