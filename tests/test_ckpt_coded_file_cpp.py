"""The host-side walks of the coded checkpoint sections (sidecar_amd/csrc/gx_ckpt_file.hpp: the
admitted (id, coding) pairs, the FIFO count table and its refusals, the FIFO coder's chunks of hosts,
the row walk at W = 514) in a stand-alone host program under AddressSanitizer and UBSan
(tests/cpp/test_ckpt_coded_file.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_ckpt_coded_file.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "build")


def test_ckpt_coded_file_host_program(tmp_path):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "test_ckpt_coded_file")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", SRC, "-o", exe], check=True)
    r = subprocess.run([exe, str(tmp_path / "scratch.gxck")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "failures=0" in r.stdout
