"""Kernel-by-kernel comparison of the gfx950 code in two sets of object files:
python tools/kernel_identity.py --old a.o [b.o ...] --new c.o [d.o ...] [--match attn]
For every kernel (by symbol): the resource row of the code object's metadata
(VGPRs, AGPRs, SGPRs, static LDS, scratch, spills) and a digest of the
disassembled instruction text (addresses, encodings and comments stripped).
Prints the symbols only one side has, the kernels whose row or text differs,
and the counts. Needs the ROCm LLVM tools (clang-offload-bundler, llvm-objdump,
llvm-readelf)."""
import argparse
import hashlib
import os
import re
import subprocess
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
          ".vgpr_spill_count", ".sgpr_spill_count", ".max_flat_workgroup_size")


def code_object(obj, tmp):
    stem = os.path.join(tmp, os.path.basename(obj) + f".{len(os.listdir(tmp))}")
    fat, out = stem + ".fatbin", stem + ".co"
    subprocess.run([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", obj, os.devnull], check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", "--unbundle", f"--input={fat}", f"--output={out}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], check=True)
    return out


def kernels(objs, match):
    """symbol -> (resource row, instruction digest, instruction count)"""
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for obj in objs:
            co = code_object(obj, tmp)
            notes = subprocess.check_output([f"{LLVM}/llvm-readelf", "--notes", co], text=True)
            rows = {}
            for blk in re.split(r"\n\s*- \.agpr_count:", "\n" + notes)[1:]:
                blk = "- .agpr_count:" + blk
                name = re.search(r"\.name:\s+(\S+)", blk).group(1)
                rows[name] = tuple(int(re.search(re.escape(f) + r":\s+(\d+)", blk).group(1)) if f in blk else -1
                                   for f in FIELDS)
            dis = subprocess.check_output([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co],
                                          text=True)
            cur, text = None, {}
            for line in dis.split("\n"):
                m = re.match(r"^[0-9a-f]* ?<([^>]+)>:$", line.strip())
                if m:
                    cur = m.group(1)
                    text[cur] = []
                elif cur and line.strip() and line.strip() != "...":   # "...": zero fill after a section's last kernel
                    text[cur].append(re.sub(r"\s*//.*$", "", line).strip())
            for name, row in rows.items():
                if match in name:
                    body = text.get(name, [])
                    res[name] = (row, hashlib.sha256("\n".join(body).encode()).hexdigest()[:16], len(body))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("--match", default="")
    a = ap.parse_args()
    old, new = kernels(a.old, a.match), kernels(a.new, a.match)
    print(f"kernels: old {len(old)}, new {len(new)}")
    for name in sorted(set(old) - set(new)):
        print("only old:", name)
    for name in sorted(set(new) - set(old)):
        print("only new:", name)
    print("fields:", " ".join(f.lstrip(".") for f in FIELDS), "| instructions | text digest")
    nrow = ntext = 0
    for name in sorted(set(old) & set(new)):
        (ro, do, no), (rn, dn, nn) = old[name], new[name]
        same_row, same_text = ro == rn, do == dn
        nrow += not same_row
        ntext += not same_text
        if same_row and same_text:   # one line for an identical kernel, both sides for one that differs
            print(f"same {name} {ro} | {no} | {do}")
        else:
            print(f"DIFF {name}\n     old {ro} | {no} | {do}\n     new {rn} | {nn} | {dn}")
    print(f"common {len(set(old) & set(new))}: resource rows differ in {nrow}, instruction text differs in {ntext}")


if __name__ == "__main__":
    main()
