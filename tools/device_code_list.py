"""The gfx950 device code of the conv / GEMM translation units, kernel by kernel: [{"tu", "name", "size", "sha256"}] of every function symbol
of each code object, compiled with the flags of imagen-pytorch_amd/build_ext.py.  Two trees whose lists are equal launch the same machine code,
which is what a host-side refactor of the launchers has to show (profiles/conv_launchers_device_code_{parent,head}.json).

    python tools/device_code_list.py [--root TREE] --out LIST.json"""
import argparse
import hashlib
import json
import os
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

TUS = ["igemm", "conv_dma", "conv_stream", "conv_pw", "conv_big", "conv_pro", "conv_gemm", "conv_small"]
LLVM = "/opt/rocm/lib/llvm/bin"


def kernels_of(root, tu, tmp):
    co = os.path.join(tmp, tu + ".co")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--offload-device-only", "--no-gpu-bundle-output", "-I" + os.path.join(root, "include"),
                    "-I" + os.path.join(root, "imagen-pytorch_amd", "csrc"), "-c", os.path.join(root, "imagen-pytorch_amd", "csrc", tu + ".hip"), "-o", co], check=True)
    text = None
    for line in subprocess.run([LLVM + "/llvm-readelf", "-S", "-W", co], check=True, capture_output=True, text=True).stdout.splitlines():
        f = line.replace("[", " ").replace("]", " ").split()
        if len(f) > 5 and f[1] == ".text":
            text = (int(f[3], 16), int(f[4], 16))   # address, file offset
    blob = open(co, "rb").read()
    rows, seen = [], set()
    for line in subprocess.run([LLVM + "/llvm-readelf", "-s", "-W", co], check=True, capture_output=True, text=True).stdout.splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC" and f[6] != "UND" and f[7] not in seen:   # (.dynsym and .symtab list the same kernels)
            seen.add(f[7])
            addr, size = int(f[1], 16), int(f[2])
            off = addr - text[0] + text[1]
            rows.append({"tu": tu, "name": f[7], "size": size, "sha256": hashlib.sha256(blob[off:off + size]).hexdigest()})
    return sorted(rows, key=lambda r: r["name"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(len(TUS)) as ex:
        rows = [r for rs in ex.map(lambda t: kernels_of(a.root, t, tmp), TUS) for r in rs]
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=0)
        f.write("\n")
    print(f"{len(rows)} kernels of {len(TUS)} translation units -> {a.out}")


if __name__ == "__main__":
    main()
