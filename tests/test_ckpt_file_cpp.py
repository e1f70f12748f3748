"""The checkpoint file's host side (sidecar_amd/csrc/gx_ckpt_file.hpp: checksum, header and table,
refusals, fork rule, record walk) in a stand-alone host program under AddressSanitizer and UBSan
(tests/cpp/test_ckpt_file.cpp), and its checksum against the numpy reference's."""
import os
import subprocess

from tests import ckpt_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_ckpt_file.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "build")


def _mix(i, seed):
    m = (i ^ ((seed * 0x9E3779B97F4A7C15) & ckpt_ref.MAXU64)) & ckpt_ref.MAXU64
    m ^= m >> 32
    m = (m * 0xD6E8FEB86659FD93) & ckpt_ref.MAXU64
    return m ^ (m >> 32)


def test_ckpt_file_host_program(tmp_path):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "test_ckpt_file")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", SRC, "-o", exe], check=True)
    sums = tmp_path / "sums.txt"
    r = subprocess.run([exe, str(tmp_path / "scratch.gxck"), str(sums)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "failures=0" in r.stdout
    # the program's checksums of its byte strings = the reference's
    for line in sums.read_text().split("\n"):
        if not line:
            continue
        n, want = map(int, line.split())
        data = bytes((_mix(i, 3) >> 24) & 0xFF for i in range(n))
        assert ckpt_ref.checksum(data) == want, n
