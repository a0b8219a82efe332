"""What the ISA tests of csrc/attn.hip share (test_kv16_isa.py, test_share_isa.py): hipcc cross-compiles a unit for gfx950 without a GPU,
once per unit name and process, and the kernels are read off the assembly text."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ssr-speech_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@functools.lru_cache(maxsize=None)
def compile_unit(name):
    """the device assembly of csrc/<name>.hip, compiled with the Makefile's code-generation flags"""
    with tempfile.TemporaryDirectory(prefix="isa_") as tmp:
        out = os.path.join(tmp, name + ".s")
        cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", f"-I{ROOT}/include", f"-I{CSRC}", "-ffp-contract=off", "-S", "--cuda-device-only",
               os.path.join(CSRC, name + ".hip"), "-o", out]
        subprocess.run(cmd, check=True, capture_output=True, timeout=600)
        with open(out) as f:
            return f.read()


def kernel_meta(asm):
    """symbol -> (vgpr_count, private_segment_fixed_size, group_segment_fixed_size) from the .amdhsa metadata"""
    meta = {}
    for m in re.finditer(r"^  - \.agpr_count:.*?(?=^  - \.agpr_count:|^amdhsa\.target:)", asm, re.S | re.M):
        t = m.group(0)
        g = lambda key: int(re.search(key + r":\s+(\d+)", t).group(1))
        meta[re.search(r"\.name:\s+(\S+)", t).group(1)] = (g(r"\.vgpr_count"), g(r"\.private_segment_fixed_size"), g(r"\.group_segment_fixed_size"))
    return meta


def sym(meta, piece):
    """the one symbol whose mangled name contains `piece`"""
    found = [k for k in meta if piece in k]
    assert len(found) == 1, (piece, found)
    return found[0]


def body(asm, symbol):
    start = asm.index("\n" + symbol + ":")
    return asm[start:asm.index(".Lfunc_end", start)]


def loads(body_text, width):
    return len(re.findall(rf"^\s+global_load_dword{width}\b", body_text, re.M))
