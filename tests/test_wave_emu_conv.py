"""CPU tier: the encoder's convolution kernels - k_enc_mid_fwd / k_enc_mid_bwd_data / k_enc_mid_wrw<16 | 8> (csrc/vae_conv_mid.h),
k_enc_stem_fwd / k_enc_stem_wrw / k_enc_stem_wrw_mfma<true | false> (csrc/vae_conv_edge.h) - as the product's own __global__
functions on emulated workgroups (tests/hostsim/wave_emu.h, wave_emu_conv.cpp): the per-frame cases of tests/parity_cases.py
against the float64 reference _conv_ref64, under the bars of the GPU tier (VAE_STEP_TOL).  What the card forgives on purpose is
explicit here: a buffer access out of range is counted (zeros loaded, store dropped) and every case asserts the counts the kernel
text determines; an access inside its resource is a plain access (a resource too long: the sanitizer child); an LDS read is the
real read, 0 at the out-of-range base, or an abort.  The grids and the 32-bit-offset gate come from the functions kvae_vae.hip
calls; test-only setters lower the persistent-grid caps so that second and third rounds run at a few frames, and choose the stem's
weight-gradient kernel as KVAE_STEM_MFMA does.  Every case asserts from the launch counters which kernel instance ran.  The
sanitizer runs are a stand-alone driver (tests/hostsim/conv_asan_driver.cpp), built once with AddressSanitizer + UBSan and once
with ThreadSanitizer, with every operand ending where its heap block ends."""
import ctypes as C
import os
import subprocess
import threading
from pathlib import Path

import pytest
import torch

import parity_cases as pc
from hostsim.build import build as build_hostsim

torch.set_num_threads(4)
ROOT = Path(__file__).resolve().parents[1]
DEV = "cpu"

# names of kvae_wemu_rnn_launches(46 ..): one per kernel instance (wave_emu_conv.cpp)
COUNTERS = ["mid.fwd<16>", "mid.fwd<8>", "mid.data<16>", "mid.data<8>", "mid.wrw<16>", "mid.wrw<8>", "stem.fwd", "stem.wrw",
            "stem.wrw_mfma<true>", "stem.wrw_mfma<false>"]
FIRST_COUNTER = 46
# setter -> the product's constant (or default of its environment switch) it stands for
SETTERS = {"kvae_wemu_enc_mid_max_wgs": 256, "kvae_wemu_stem_max_rows": 1024, "kvae_wemu_stem_mode": 1}
STEM_KERNEL = {0: "stem.wrw", 1: "stem.wrw_mfma<true>", 2: "stem.wrw_mfma<false>"}   # KVAE_STEM_MFMA -> instance (1: with mask words)
SANITIZERS = {"asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"],
              "tsan": ["-fsanitize=thread"]}
KVAE_ERR_ARG = 4


@pytest.fixture(scope="module", autouse=True)
def wave_emu_backend():
    from kvae import _native
    lib = _native.LgssmLib(build_hostsim())
    d = lib.dll
    d.kvae_wemu_enc_mid_gate.argtypes = [C.c_int64, C.c_int32]
    d.kvae_wemu_conv_oob.argtypes = [C.c_int, C.c_int]
    d.kvae_wemu_conv_oob.restype = C.c_long
    _native._set_test_backend(lib)
    d.kvae_hostsim_wave_emu(1)
    yield lib
    d.kvae_hostsim_wave_emu(0)
    _native._set_test_backend(None)


@pytest.fixture(autouse=True)
def product_caps(wave_emu_backend):
    yield
    for name in SETTERS:
        getattr(wave_emu_backend.dll, name)(-1)


@pytest.fixture(scope="module", autouse=True)
def sanitizer_runs(tmp_path_factory):
    """The two builds and runs of the sanitizer driver go on in threads of their own while the cases of this file run, so that the
    file costs the longest of them, not the sum; test_kernels_under_sanitizers collects them."""
    src = ROOT / "tests" / "hostsim" / "conv_asan_driver.cpp"
    res = {}

    def work(tag):
        out = tmp_path_factory.mktemp("conv_" + tag) / ("conv_driver_" + tag)
        try:
            subprocess.run(["g++", "-std=c++17", "-O1", "-g1", "-pthread", "-Wno-psabi", *SANITIZERS[tag], "-I",
                            str(ROOT / "tests" / "hostsim" / "stub"), "-o", str(out), str(src)], check=True, cwd=ROOT,
                           capture_output=True, text=True)
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


def mid_oob(N, side, grid):
    """{instance: (loads answered with zeros, stores dropped)} of ONE launch of each enc_mid kernel, per lane access of 16 bytes,
    read off the kernel text.  Every workgroup fetches, besides its own iterations, the one a whole round past its last - all of
    it past the end: 16 pieces of `in` (forward), 4 + 4 of g_out / out (data gradient), all 24 (weight gradient), 256 lanes each.
    The first flush of a workgroup (4 stores per lane forward, 16 in the data gradient) has no image yet and goes to offset 2^31.
    A ragged last iteration loads zeros for, and drops the results of, its frames >= N.  The weight gradient stores plainly."""
    fpi, frame, oframe = (2, 32 * 256, 32 * 64) if side == 16 else (8, 32 * 64, 32 * 16)
    ragged = -N % fpi
    s = "<%d>" % side
    return {"mid.fwd" + s: (grid * 4096 + ragged * frame // 4, grid * 1024 + ragged * oframe // 4),
            "mid.data" + s: (grid * 2048 + 2 * ragged * oframe // 4, grid * 4096 + ragged * frame // 4),
            "mid.wrw" + s: (grid * 6144 + ragged * (frame + 2 * oframe) // 4, 0)}


class Routed:
    """with Routed(lib, {"mid.fwd<16>": 1, ...}, oob={...}): ... - the emulated launches of the block, all of them, by kernel
    instance; `oob`: the out-of-range counts of each named instance's last launch."""

    def __init__(self, lib, want, oob=None):
        self.lib, self.want, self.oob = lib, {k: v for k, v in want.items() if v}, oob or {}
        assert set(self.want) <= set(COUNTERS) and set(self.oob) <= set(self.want), (self.want, self.oob)

    def counts(self):
        return [self.lib.dll.kvae_wemu_rnn_launches(FIRST_COUNTER + i) for i in range(len(COUNTERS))]

    def __enter__(self):
        self.before = self.counts()
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            got = {n: a - b for n, a, b in zip(COUNTERS, self.counts(), self.before) if a != b}
            assert got == self.want, (got, self.want)
            for name, want in self.oob.items():
                i = FIRST_COUNTER + COUNTERS.index(name)
                got = (self.lib.dll.kvae_wemu_conv_oob(i, 0), self.lib.dll.kvae_wemu_conv_oob(i, 1))
                assert got == want, (name, "zeroed loads, dropped stores", got, want)


class Setting:
    """with Setting(lib, "kvae_wemu_enc_mid_max_wgs", 2): ... - a launch-geometry argument set for the block."""

    def __init__(self, lib, name, value):
        self.fn, self.value = getattr(lib.dll, name), value

    def __enter__(self):
        self.fn(self.value)

    def __exit__(self, *a):
        self.fn(-1)


def _mid_launches(side, runs=1, data=None):
    s = "<%d>" % side
    return {"mid.fwd" + s: runs, "mid.data" + s: runs if data is None else data, "mid.wrw" + s: runs}


def _mid_case(lib, N, side, grid):
    """One conv_layer_per_frame case of enc_mid: `grid` workgroups, one launch of each kernel, the counts of mid_oob."""
    assert lib.dll.kvae_enc_mid_partial_rows(N, side) == grid
    with Routed(lib, _mid_launches(side), mid_oob(N, side, grid)):
        return pc.conv_layer_per_frame(DEV, "enc_mid", N, side)


# ---- residues of the frames per iteration ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("side,N", [(16, n) for n in (1, 2, 3, 5)] + [(8, n) for n in (1, 7, 8, 9, 13, 17)])
def test_enc_mid_residues(wave_emu_backend, side, N):
    fpi = 2 if side == 16 else 8
    _mid_case(wave_emu_backend, N, side, (N + fpi - 1) // fpi)


@pytest.mark.parametrize("N", [1, 2, 3])
def test_stem_residues(wave_emu_backend, N):
    """Through the fused Function on the host there are no mask words: the default mode takes k_enc_stem_wrw_mfma<false>."""
    with Routed(wave_emu_backend, {"stem.fwd": 1, "stem.wrw_mfma<false>": 1}, {"stem.fwd": (0, 0), "stem.wrw_mfma<false>": (0, 0)}):
        pc.conv_layer_per_frame(DEV, "stem", N, 32)


# ---- persistent rounds ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side,N", [(16, 9), (8, 33)])
@pytest.mark.parametrize("cap", [2, 3])
def test_enc_mid_persistent_rounds(wave_emu_backend, side, N, cap):
    """Five iterations (the last one ragged) on `cap` workgroups.  Cap 2: workgroup 0 runs three - two flushes of a finished image
    inside the loop, a prefetch past the end on its last - and workgroup 1 two; cap 3: two, two and one."""
    lib = wave_emu_backend
    with Setting(lib, "kvae_wemu_enc_mid_max_wgs", cap):
        _mid_case(lib, N, side, cap)
    assert lib.dll.kvae_enc_mid_partial_rows(N, side) == 5


@pytest.mark.parametrize("side,N", [(16, 33), (8, 129)])
def test_enc_mid_every_rotation(wave_emu_backend, side, N):
    """17 workgroups: rot = blockIdx.x & 15 takes 0 .. 15 and 0 again, the last iteration ragged."""
    _mid_case(wave_emu_backend, N, side, 17)


# ---- the stem's three weight-gradient kernels on the same inputs ------------------------------------------------------------------
def _stem_variants(lib, N, cap):
    from kvae import _native as Nt
    from kvae.vae import fused
    d = lib.dll
    for draw in range(8):
        x, s, W, b, gh = pc._vae_inputs("stem", N, 32, 11 + 1000 * draw, "cpu", False)
        want, up, near = pc._vae_reference("stem", x, s, W, b, lambda near: torch.randn(near.shape, generator=gh) * ~near)
        if float(near.double().mean()) <= pc.VAE_NEAR_SHARE:
            break
    assert float(near.double().mean()) <= pc.VAE_NEAR_SHARE
    out = torch.empty(N, 32, 16, 16)
    bits = torch.empty(N, 256, dtype=torch.int32)
    with Routed(lib, {"stem.fwd": 1}):
        lib.check(d.kvae_enc_stem_fwd(Nt.ptr(x), Nt.ptr(W), Nt.ptr(b), Nt.ptr(out), Nt.ptr(bits), N, 32, 32, None), "kvae_enc_stem_fwd")
    pc._vae_check_mask(out, want[0], near)
    sign = ((bits.view(N, 1, 16, 16) >> torch.arange(32, dtype=torch.int32).view(1, 32, 1, 1)) & 1).bool()
    assert not bool(((sign != (want[0] > 0)) & ~near).any()), "the mask words differ from float64 away from the threshold"
    got = {}
    with Setting(lib, "kvae_wemu_stem_max_rows", cap):
        rows = d.kvae_conv_edge_partial_rows(N)
        assert rows == (min(N, cap) if cap > 0 else N)
        for mode, name in STEM_KERNEL.items():
            wp, bp = torch.full((rows, 288), float("nan")), torch.full((rows, 32), float("nan"))
            with Setting(lib, "kvae_wemu_stem_mode", mode), Routed(lib, {name: 1}, {name: (0, 0)}):
                # mode 1 is given the mask words and NO activation; the other two the activation and no words
                lib.check(d.kvae_enc_stem_bwd(Nt.ptr(x), None if mode == 1 else Nt.ptr(out), Nt.ptr(bits) if mode == 1 else None,
                                              Nt.ptr(up.contiguous()), Nt.ptr(wp), Nt.ptr(bp), N, 32, 32, None), "kvae_enc_stem_bwd")
            gw, gb = fused.colsum_pair(wp, bp)
            res = {}
            pc._vae_compare("stem", (out, None, gw.view(32, 1, 3, 3), gb), want, res)   # each under its own bar
            got[mode] = (gw, gb)
    # <true> and <false> differ only in where the mask comes from: away from the threshold (no upstream gradient there) the same bits
    assert torch.equal(got[1][0], got[2][0]) and torch.equal(got[1][1], got[2][1])


@pytest.mark.parametrize("N,cap", [(3, -1), (5, 2)])
def test_stem_variants_agree(wave_emu_backend, N, cap):
    """k_enc_stem_wrw, k_enc_stem_wrw_mfma<true> (on the mask words the emulated forward wrote) and <false>: one workgroup per frame,
    and five frames on two workgroups - three rounds and two, the prefetch of frame n + 2 past the end on the last of each."""
    _stem_variants(wave_emu_backend, N, cap)


def test_stem_bwd_refuses_without_mask(wave_emu_backend):
    """Neither activation nor mask words: KVAE_ERR_NULL from the argument check; words only in a mode that needs the activation:
    KVAE_ERR_NULL from es_wrw_kernel - and no launch either way."""
    from kvae import _native as Nt
    lib = wave_emu_backend
    t = torch.zeros(1, 32, 16, 16)
    x, wp, bp, bits = torch.zeros(1, 1, 32, 32), torch.zeros(1, 288), torch.zeros(1, 32), torch.zeros(1, 256, dtype=torch.int32)
    with Routed(lib, {}):
        assert lib.dll.kvae_enc_stem_bwd(Nt.ptr(x), None, None, Nt.ptr(t), Nt.ptr(wp), Nt.ptr(bp), 1, 32, 32, None) == 2
        for mode in (0, 2):
            with Setting(lib, "kvae_wemu_stem_mode", mode):
                assert lib.dll.kvae_enc_stem_bwd(Nt.ptr(x), None, Nt.ptr(bits), Nt.ptr(t), Nt.ptr(wp), Nt.ptr(bp), 1, 32, 32, None) == 2


# ---- structure ------------------------------------------------------------------------------------------------------------------
def _probe_params():
    for layer, side in (("enc_mid", 16), ("enc_mid", 8), ("stem", 32)):
        for kind in ("upstream", "input"):
            for frame in pc.probe_frames(layer, side)[1]:
                yield layer, side, kind, frame


@pytest.mark.parametrize("layer,side,kind,frame", list(_probe_params()))
def test_conv_probes(wave_emu_backend, layer, side, kind, frame):
    """One upstream gradient pixel (the data gradient exactly zero outside its receptive field) / one input pixel (every other
    frame exactly relu(bias)): nine positions of one frame of probe_frames - the first and the last frame of an iteration, the
    last frame of a ragged one."""
    probes = [p for p in pc.vae_probe_cases(layer, side) if p[0] == kind and p[1] == frame]
    assert len(probes) == 9
    N = pc.probe_frames(layer, side)[0]
    if layer == "stem":
        want, oob = {"stem.fwd": 9, "stem.wrw_mfma<false>": 9}, {}
    else:
        grid = (N + (2 if side == 16 else 8) - 1) // (2 if side == 16 else 8)
        want, oob = _mid_launches(side, 9), mid_oob(N, side, grid)
    with Routed(wave_emu_backend, want, oob):
        for k, f, pos in probes:
            pc.conv_probe(DEV, layer, side, k, f, pos)


@pytest.mark.parametrize("side,N", [(16, 5), (8, 13)])
def test_enc_mid_without_input_gradient(wave_emu_backend, side, N):
    """g_in = NULL: no data-gradient launch, the same weight and bias gradients bit for bit."""
    fpi = 2 if side == 16 else 8
    oob = mid_oob(N, side, (N + fpi - 1) // fpi)
    with Routed(wave_emu_backend, _mid_launches(side, 2, data=1), oob):
        pc.conv_no_input_grad(DEV, "enc_mid", N, side)


def test_stem_valu_kernel_through_the_function(wave_emu_backend):
    """KVAE_STEM_MFMA = 0 through the fused Function: k_enc_stem_wrw, three frames on two workgroups."""
    lib = wave_emu_backend
    with Setting(lib, "kvae_wemu_stem_mode", 0), Setting(lib, "kvae_wemu_stem_max_rows", 2), Routed(lib, {"stem.fwd": 1, "stem.wrw": 1}):
        pc.conv_layer_per_frame(DEV, "stem", 3, 32)


# ---- the refusal ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side,largest", [(16, 63487), (8, 260095)])
def test_enc_mid_offset_gate(wave_emu_backend, side, largest):
    """em_launch_ok, the gate kvae_enc_mid_fwd / bwd apply (no launch here).  The farthest byte a launch computes an offset for is
    the prefetch a whole round of 256 iterations of at most 8 frames past the end: (N + 2048) frames x 32 x side^2 x 4 bytes must
    stay below 2^31 - `largest` is the last N for which it does."""
    assert (largest + 2048) * 32 * side * side * 4 < 2 ** 31 <= (largest + 1 + 2048) * 32 * side * side * 4
    gate = wave_emu_backend.dll.kvae_wemu_enc_mid_gate
    with Routed(wave_emu_backend, {}):
        assert gate(largest, side) == 0 and gate(largest + 1, side) == KVAE_ERR_ARG
        assert gate(0, side) == KVAE_ERR_ARG and gate(1, side) == 0
        t = torch.zeros(8)   # the entry points refuse before they look at a single element
        from kvae import _native as Nt
        p = Nt.ptr(t)
        assert wave_emu_backend.dll.kvae_enc_mid_fwd(p, p, p, p, largest + 1, 32, side, None) == KVAE_ERR_ARG
        assert wave_emu_backend.dll.kvae_enc_mid_bwd(p, p, p, p, p, p, p, largest + 1, 32, side, None) == KVAE_ERR_ARG


# ---- the tier itself ------------------------------------------------------------------------------------------------------------
def test_emulator_selftest(wave_emu_backend):
    """The 32x32x2 map against a triple loop, buffer accesses inside / outside their resource (and the classification of a
    straddling one), the three outcomes of an LDS read that may leave the allocation - with the emulator's earlier cases."""
    assert wave_emu_backend.dll.kvae_wemu_selftest() == 0


def test_setters_hold_the_product_constants(wave_emu_backend):
    """A setter returns the value it replaces: without a test's setting that is the constant kvae_vae.hip passes."""
    for name, constant in SETTERS.items():
        fn = getattr(wave_emu_backend.dll, name)
        assert fn(7) == constant and fn(-1) == 7 and fn(-1) == constant, name
    assert wave_emu_backend.dll.kvae_enc_mid_partial_rows(10 ** 4, 16) == 256 and wave_emu_backend.dll.kvae_conv_edge_partial_rows(10 ** 4) == 1024


def test_off_means_the_plain_twins(wave_emu_backend):
    """With the emulation off the host simulation is what it was: the plain-loop twins, no emulated launch, caps ignored."""
    lib = wave_emu_backend
    lib.dll.kvae_hostsim_wave_emu(0)
    try:
        with Routed(lib, {}), Setting(lib, "kvae_wemu_enc_mid_max_wgs", 2), Setting(lib, "kvae_wemu_stem_max_rows", 2):
            assert lib.dll.kvae_enc_mid_partial_rows(9, 16) == 5 and lib.dll.kvae_conv_edge_partial_rows(5) == 5
            pc.conv_layer_per_frame(DEV, "enc_mid", 9, 16)
            pc.conv_layer_per_frame(DEV, "enc_mid", 9, 8)
            pc.conv_layer_per_frame(DEV, "stem", 5, 32)
    finally:
        lib.dll.kvae_hostsim_wave_emu(1)


@pytest.mark.parametrize("tag", list(SANITIZERS))
def test_kernels_under_sanitizers(sanitizer_runs, tag):
    """The same kernels in a stand-alone program (tests/hostsim/conv_asan_driver.cpp) run as a child process, at the residue and the
    capped-round shapes above: with -fsanitize=address,undefined every operand ends where its heap block ends, every buffer access
    below num_records is a plain access and every LDS array has its exact size; with -fsanitize=thread the LDS images that leave
    during the next iteration are checked against the barriers that protect them.  (Built and run beside the cases above.)"""
    sanitizer_runs["threads"][tag].join()
    assert tag + "-error" not in sanitizer_runs, sanitizer_runs.get(tag + "-error")
    r = sanitizer_runs[tag]
    assert r.returncode == 0 and "CONV-SAN-OK" in r.stdout and "Sanitizer" not in r.stderr, r.stdout[-2000:] + r.stderr[-6000:]
