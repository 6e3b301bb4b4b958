#!/usr/bin/env python3
"""Instruction mix of K1's row kernels from the gfx950 cross-compile (no GPU).

Compiles hhfm_amd/csrc/fm_rows.hip (or the file given with --src) to device
assembly and, for every kernel whose demangled name contains --kernel, prints
VGPRs, scratch and, for its largest loops (the blocks the compiler annotates
with one loop header; in fm_rows_fast_hot the LDS-tail loop, then the general
loop), the counts the consume phase is judged by: VALU, DPP-folded
VALU, ds_bpermute_b32, other LDS, s_waitcnt, s_nop, global loads / stores,
64-bit compares, scalar dword loads (the user / item `w` of the LDS-tail loop),
v_readlane / v_writelane (SGPR spill traffic shows up as more of these than the
`w` path's own) and the s_waitcnt that drain lgkmcnt to 0.

  python scripts/k1_isa_mix.py --kernel "fm_rows_fast_hot<5, 16, false, true, true>"
"""
import argparse
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def functions(asm):
    """{mangled name: [lines]} of every .type @function body"""
    out, name, body = {}, None, []
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is not None:
            body.append(line)
            if line.strip().startswith(".end_amdhsa_kernel"):
                out[name] = body
                name = None
    return out


def loops(body):
    """{loop header block: [lines]} from the compiler's block annotations
    ("=>This Inner Loop Header" / "in Loop: Header=BBn_m")"""
    out, cur = {}, None
    for l in body:
        if re.match(r"^(\.LBB\w+:|; %bb\.\d+:)", l):
            m = re.search(r"in Loop: Header=(BB\w+)", l)
            if m:
                cur = m.group(1)
            elif "Loop Header" in l:
                cur = l.split(":")[0].lstrip(".L")
            else:
                cur = None
            continue
        if cur is not None:
            out.setdefault(cur, []).append(l)
    return out


def mix(lines):
    ins = [l.split()[0] for l in lines if re.match(r"^\s+[a-z]\w+", l) and not l.strip().startswith(".")]
    n = lambda pred: sum(1 for i in ins if pred(i))
    return {
        "instructions": len(ins),
        "VALU": n(lambda i: i.startswith("v_")),
        "VALU_dpp": n(lambda i: i.startswith("v_") and i.endswith("_dpp")),
        "ds_bpermute": n(lambda i: i.startswith("ds_bpermute")),
        "LDS_other": n(lambda i: i.startswith("ds_") and not i.startswith("ds_bpermute")),
        "s_waitcnt": n(lambda i: i == "s_waitcnt"),
        "s_nop": n(lambda i: i == "s_nop"),
        "global_load_dwordx4": n(lambda i: i == "global_load_dwordx4"),
        "global_load_dword": n(lambda i: i == "global_load_dword"),
        "global_store": n(lambda i: i.startswith("global_store")),
        "s_load_dword": n(lambda i: i == "s_load_dword"),
        "s_load_wide": n(lambda i: i.startswith("s_load_dwordx")),
        "v_readlane": n(lambda i: i.startswith("v_readlane")),
        "v_writelane": n(lambda i: i.startswith("v_writelane")),
        "lgkmcnt0": sum(1 for l in lines if re.match(r"^\s+s_waitcnt\b.*lgkmcnt\(0\)", l)),
        "v_cmp_u64": n(lambda i: re.match(r"v_cmp\w*_u64", i) is not None),
        "v_cmp_i64": n(lambda i: re.match(r"v_cmp\w*_i64", i) is not None),
    }


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--src", default=os.path.join(ROOT, "hhfm_amd", "csrc", "fm_rows.hip"))
    p.add_argument("--asm", default=None, help="use this assembly file instead of compiling")
    p.add_argument("--kernel", default="fm_rows_fast_hot<5, 16, false, true, true>")
    p.add_argument("--defs", default="", help="extra -D flags")
    p.add_argument("--loops", type=int, default=2, help="largest loops to print per kernel")
    a = p.parse_args()
    if a.asm:
        asm = open(a.asm).read()
    else:
        with tempfile.TemporaryDirectory() as tmp:
            s = os.path.join(tmp, "k.s")
            subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                            "--cuda-device-only", "-S", *a.defs.split(), a.src, "-o", s], check=True)
            asm = open(s).read()
    fns = functions(asm)
    names = list(fns)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True,
                         check=True).stdout.splitlines()
    for name, d in zip(names, dem):
        if a.kernel not in d:
            continue
        body = fns[name]
        text = "\n".join(body)
        vg = re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", text)
        acc = re.search(r"\.amdhsa_accum_offset\s+(\d+)", text)
        scr = re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", text)
        print(d.replace("hhfm::", ""))
        print(f"  next_free_vgpr {vg.group(1) if vg else '?'}  accum_offset "
              f"{acc.group(1) if acc else '?'}  scratch {scr.group(1) if scr else '?'}")
        found = sorted(loops(body).items(), key=lambda kv: -len(kv[1]))
        for header, lines in found[:a.loops]:
            print(f"  loop {header}: {mix(lines)}")


if __name__ == "__main__":
    main()
