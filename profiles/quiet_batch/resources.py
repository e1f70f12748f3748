"""Registers, scratch, LDS, occupancy and code size of k_send's planned instances without listeners
(gfx950), from a build log with the compiler's resource remarks and from the library's symbol sizes.

  hipcc ... -Rpass-analysis=kernel-resource-usage -o libgx.so ... 2> build.txt
  python profiles/quiet_batch/resources.py build.txt libgx.so > resources.jsonl"""
import json
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
# k_send<T, X, SCAN, VEC, EV, OWN, PLAN, QUIET>
NAME = re.compile(r"_Z6k_sendILi4ELb0ELb([01])ELb([01])ELb0ELi(\d)ELb1ELb([01])EEv3Dev\w*")
FIELDS = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "waves_per_simd",
          "SGPRs Spill": "sgpr_spills", "LDS Size [bytes/block]": "lds"}


def remarks(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {}) if NAME.fullmatch(m.group(1)) else None
            continue
        m = re.search(r"remark:\s+([^:]+): (\d+) \[", line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[FIELDS[m.group(1)]] = int(m.group(2))
    return out


def code_sizes(lib):
    with tempfile.TemporaryDirectory() as tmp:
        co = os.path.join(tmp, "gfx950.co")
        sec = os.path.join(tmp, "fatbin")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, sec], check=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--allow-missing-bundles",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={sec}", f"--output={co}"], check=True)
        txt = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-s", "-W", co], check=True, stdout=subprocess.PIPE).stdout.decode()
    sizes = {}
    for line in txt.splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC" and NAME.fullmatch(f[7]):
            sizes[f[7]] = max(sizes.get(f[7], 0), int(f[2]))
    return sizes


if __name__ == "__main__":
    rem, sizes = remarks(sys.argv[1]), code_sizes(sys.argv[2])
    rows = []
    for name, r in rem.items():
        scan, vec, own, quiet = (int(x) for x in NAME.fullmatch(name).groups())
        rows.append(dict(scan=scan, vec=vec, own=own, quiet=quiet, **r, code_bytes=sizes.get(name)))
    for row in sorted(rows, key=lambda x: (x["scan"], x["vec"], x["own"], x["quiet"])):
        print(json.dumps(row))
