"""CPU tier: the 64-lane form of the ELBO bodies (csrc/lgssm_elbo.h) on emulated wavefronts, under AddressSanitizer +
UndefinedBehaviorSanitizer and under ThreadSanitizer.  tests/hostsim/elbo_wave_driver.cpp is a program of its own (nothing is
loaded into Python): it runs elbo_probe_body + elbo_body with lanes striding KV_PAR, KV_LANE0 sections and KV_SYNC() as the
emulator's rendezvous, one emulated wavefront per (b,t), and compares every output bit for bit with the serial host build of the
same bodies.  The emulator's lanes are host threads and its rendezvous a mutex and a condition variable, so ThreadSanitizer
reports an LDS element that one lane writes and another reads inside one phase - a missing KV_SYNC(), a side effect outside
KV_LANE0 - as a data race: the phase rules at the top of csrc/lgssm_vm.h, which no other CPU test can see."""
import os
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HOSTSIM = ROOT / "tests" / "hostsim"


@pytest.mark.parametrize("tag,flags", [("asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]),
                                       ("tsan", ["-fsanitize=thread"])])
def test_elbo_bodies_on_emulated_wavefronts(tag, flags):
    """SDims<4,4,2>, SDims<16,16,2> and RDims at (5,3,2) and (16,16,16); B = 2, T = 1, 2, 3; with and without gradients, with and
    without ws_lz, levels (0,0), (2,0), (5,5), a per-step and a shared Q, a mask."""
    src, out, obj = HOSTSIM / "elbo_wave_driver.cpp", HOSTSIM / f"elbo_wave_driver_{tag}", HOSTSIM / f"elbo_wave_driver_{tag}_serial.o"
    cc = ["g++", "-std=c++17", "-O1", "-g", "-pthread", *flags, "-I", str(HOSTSIM / "stub")]
    subprocess.run(cc + ["-DELBO_DRIVER_SERIAL", "-c", str(src), "-o", str(obj)], check=True, cwd=ROOT)   # the serial form of the bodies
    subprocess.run(cc + [str(src), str(obj), "-o", str(out)], check=True, cwd=ROOT)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1", TSAN_OPTIONS="halt_on_error=0:exitcode=66")
    r = subprocess.run([str(out)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ELBO-WAVE-OK" in r.stdout and "Sanitizer" not in r.stderr, r.stdout[-2000:] + r.stderr[-6000:]
