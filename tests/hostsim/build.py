"""Build the TEST-ONLY host simulation of the kernel bodies (tests/hostsim/hostsim.cpp)."""
import os
import subprocess
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
SRC = HERE / "hostsim.cpp"
EMU = HERE / "wave_emu_kernels.cpp"   # the wavefront-level kernels on emulated wavefronts (wave_emu.h)
RNN = HERE / "wave_emu_rnn.cpp"       # the recurrent kernels (LSTM, bi-GRU, regime chain) on emulated workgroups
RED = HERE / "wave_emu_reduce.cpp"    # the weight-gradient, mixture and linear-head kernels on emulated workgroups
STEP = HERE / "wave_emu_step.cpp"     # clip + Adam, loss head, column sums, emission means, conv epilogues on emulated workgroups
CONV = HERE / "wave_emu_conv.cpp"     # the encoder's stride-2 and stem convolution kernels on emulated workgroups
STUB = HERE / "stub"                  # <hip/hip_runtime.h> for the kernel headers that include it unconditionally
DEPS = [SRC, EMU, RNN, RED, STEP, CONV, HERE / "wave_emu.h", STUB / "hip" / "hip_runtime.h"] + sorted((ROOT / "kalman-vae_amd" / "csrc").glob("*.h")) + [ROOT / "include" / "kvae_lgssm.h"]


def build(sanitize=False):
    out = HERE / ("libkvae_hostsim_asan.so" if sanitize else "libkvae_hostsim.so")
    if out.exists() and all(out.stat().st_mtime >= d.stat().st_mtime for d in DEPS):
        return out
    cmd = ["g++", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unknown-pragmas", "-Wno-psabi", "-pthread", "-I", str(STUB), "-o", str(out), str(SRC), str(EMU), str(RNN), str(RED), str(STEP), str(CONV)]
    cmd += ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.run(cmd, check=True, cwd=ROOT)
    return out


if __name__ == "__main__":
    print(build(), build(sanitize=True))
