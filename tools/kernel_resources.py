#!/usr/bin/env python3
"""Per-kernel resource usage (VGPR/SGPR/AGPR/LDS/spill/occupancy) from the
built extension's embedded gfx950 code objects. Works without a GPU.

The extension is linked from one translation unit per kernel family, and
each contributes its own __CLANG_OFFLOAD_BUNDLE__; all of them are read.

Occupancy on CDNA4: VGPRs+AGPRs come from one 512-register file per SIMD;
waves/SIMD ~= 512 // (vgpr+agpr rounded up to 8), capped at 8 by LDS
(160 KB/CU) and workgroup shape.

Usage: python tools/kernel_resources.py [path/to/lib.so]

Manual check after a compiler upgrade (no test sees it: every result stays
right, only the latency comes back): `k_attn_wide` must issue all loads of
a round before its first wait. Disassemble the code objects
(`llvm-objdump -d` on what extract_hsacos() returns, or hipcc `-S
--cuda-device-only` on csrc/attn.hip) and read `k_attn_wide<2, __half,
SeqRows>`: 2 q loads, then inside the loop 4 `global_load_dwordx4` (K) and
16 `global_load_dword` (V) with no `s_waitcnt vmcnt` between them, then
`; sched_barrier`, then the first wait, `s_waitcnt vmcnt(19)`. A
`vmcnt(0)` between the loads, or V loads below the barrier, is the serial
form that profiles/r07_wide_attention.md describes (4.4 -> 14 us). The Q80
forms, `k_attn_wide<V, signed char, Q80Rows<..>>`, issue 40 loads per round
the same way (4 K runs, 4 K scales, 16 V dwords, 16 V scale dwords, all but
the K runs `global_load_dword`), then `; sched_barrier`, then the first
wait, `vmcnt(39)`; a `flat_load`, a `global_load_ushort` / `_ubyte` or a
wait between those loads is the serial form again
(profiles/r09_q80_kv.md).

Second manual check: `k_q40_gemv<1, 2, 5, 0>` (the hand-off form of
q40_gemv_resid_q) exchanges rows between workgroups of one launch. Expected
here: 0 spill and no more VGPRs than `k_q40_gemv<1, 2, 1, 0>`. In its
disassembly the store of x must be a `global_store_dwordx2 ... sc1`
followed by `s_waitcnt vmcnt(0)` before the `s_barrier` in front of the
ticket's `global_atomic_add`, the load of x after the second barrier a
`global_load_dword ... sc1`, and the kernel must hold no `buffer_wbl2` and
no `buffer_inv` (profiles/r08_resid_q_handoff.md).
"""

import re
import struct
import subprocess
import sys
import os
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def extract_hsacos(so_path: str) -> list:
    """The gfx950 code object of every offload bundle in the library."""
    data = open(so_path, "rb").read()
    out = []
    off = data.find(MAGIC)
    while off >= 0:
        p = off + len(MAGIC)
        n, = struct.unpack_from("<Q", data, p)
        p += 8
        for _ in range(n):
            eoff, esz, idl = struct.unpack_from("<QQQ", data, p)
            p += 24
            ident = data[p: p + idl].decode()
            p += idl
            if "gfx950" in ident:
                out.append(data[off + eoff: off + eoff + esz])
        off = data.find(MAGIC, off + len(MAGIC))
    if not out:
        raise SystemExit(f"no gfx950 code object in {so_path}")
    return out


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names),
                         capture_output=True, text=True)
    return out.stdout.splitlines()


def kernel_notes(hsaco: bytes) -> list:
    with tempfile.NamedTemporaryFile(suffix=".hsaco") as f:
        f.write(hsaco)
        f.flush()
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", f.name],
                               capture_output=True, text=True).stdout
    kernels = []
    cur = {}
    for line in notes.splitlines():
        m = re.match(r"\s*- \.agpr_count:\s*(\d+)", line)
        if m:
            if cur:
                kernels.append(cur)
            cur = {"agpr": int(m.group(1))}
        for key, pat in (("name", r"\.name:\s*(\S+)"),
                         ("sgpr", r"\.sgpr_count:\s*(\d+)"),
                         ("vgpr", r"\.vgpr_count:\s*(\d+)"),
                         ("spill", r"\.private_segment_fixed_size:\s*(\d+)"),
                         ("lds", r"\.group_segment_fixed_size:\s*(\d+)")):
            m = re.search(pat, line)
            if m:
                cur[key] = m.group(1) if key == "name" else int(m.group(1))
    if cur:
        kernels.append(cur)
    return kernels


def main():
    so = sys.argv[1] if len(sys.argv) > 1 else os.path.join(
        os.path.dirname(os.path.abspath(__file__)), "..",
        "dllama_amd", "ops", "_build", "dllama_hip.so")
    kernels = [k for h in extract_hsacos(so) for k in kernel_notes(h)]
    names = demangle([k.get("name", "?") for k in kernels])
    print(f"{'kernel':44s} {'VGPR':>5s} {'AGPR':>5s} {'SGPR':>5s} "
          f"{'LDS':>6s} {'spill':>5s} {'waves/SIMD':>10s}")
    for k, nm in sorted(zip(kernels, names),
                        key=lambda t: (-(t[0].get("vgpr", 0) + t[0].get("agpr", 0)),
                                       t[1])):
        short = nm.split("(")[0]
        tot = k.get("vgpr", 0) + k.get("agpr", 0)
        waves = min(8, 512 // max(8, (tot + 7) // 8 * 8)) if tot else 8
        print(f"{short:44s} {k.get('vgpr', 0):5d} {k.get('agpr', 0):5d} "
              f"{k.get('sgpr', 0):5d} {k.get('lds', 0):6d} "
              f"{k.get('spill', 0):5d} {waves:10d}")


if __name__ == "__main__":
    main()
