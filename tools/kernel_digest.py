#!/usr/bin/env python3
"""Digest of every gfx950 kernel the HIP sources generate, to show that a refactor left the device code alone.

  python tools/kernel_digest.py digest SRC_DIR OUT.json [-D MACRO ...] [FILE.hip ...]   (default: every SRC_DIR/*.hip)
  python tools/kernel_digest.py compare OLD.json NEW.json

digest compiles each file device-only with the project's flags and records, per kernel symbol, the sha256 of its
instruction stream (llvm-objdump -d --no-leading-addr with the address / encoding comments cut: branch operands are
relative, so a kernel that moved to another file compares equal; the s_nop fill behind its last instruction left out) and
the resource metadata of its code-object note.
compare matches kernels by demangled name and, where a name is gone (a template head changed), by equal content."""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import yaml

ROCM = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))
META = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
        "group_segment_fixed_size", "max_flat_workgroup_size", "kernarg_segment_size")


def run(*cmd):
    r = subprocess.run([str(c) for c in cmd], capture_output=True, text=True)
    if r.returncode:
        sys.exit(r.stderr)
    return r.stdout


def digest_file(src, include, defines, tmp):
    obj, co = tmp / (src.name + ".o"), tmp / (src.name + ".co")
    run(ROCM / "bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", f"-I{include}", *defines, "-x", "hip",
        "--offload-device-only", "-c", src, "-o", obj)
    run(ROCM / "llvm/bin/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hip-amdgcn-amd-amdhsa--gfx950",
        f"--input={obj}", f"--output={co}")
    notes = run(ROCM / "llvm/bin/llvm-readelf", "--notes", co)
    meta = {k[".symbol"][:-3]: k for k in yaml.safe_load(notes[notes.index("---"):notes.rindex("...")])["amdhsa.kernels"]}
    streams, sym = {}, None
    for line in run(ROCM / "llvm/bin/llvm-objdump", "-d", "--no-leading-addr", co).splitlines():
        m = re.match(r"<(\S+)>:$", line)
        if m:
            sym = m.group(1)
            streams[sym] = []
        elif sym and line.strip() not in ("", "..."):  # "...": zero padding behind a symbol
            streams[sym].append((line.split("//")[0].rstrip(), len(line.split("//")[1].split(":")[1].split()) * 4 if "//" in line else 0))
    out = {}
    for sym, ins in streams.items():
        if sym not in meta:
            continue  # not a kernel
        # the fill behind a kernel's last instruction is not its own: up to the next symbol's alignment, and for the
        # file's last symbol the prefetch margin at the end of the section -- which kernel comes last changes with the file
        while ins and ins[-1][0].split() == ["s_nop", "0"]:
            ins.pop()
        name = run("c++filt", sym).strip()
        out[f"{src.name}::{name}"] = {"bytes": sum(b for _, b in ins), "sha": hashlib.sha256("\n".join(t for t, _ in ins).encode()).hexdigest(),
                                      **{k: meta[sym].get("." + k, 0) for k in META}}
    return out


def main():
    if sys.argv[1] == "digest":
        src_dir, out = Path(sys.argv[2]), Path(sys.argv[3])
        rest = sys.argv[4:]
        defines = [f"-D{rest[i + 1]}" for i, a in enumerate(rest) if a == "-D"]
        files = [src_dir / a for i, a in enumerate(rest) if a != "-D" and (i == 0 or rest[i - 1] != "-D")] or sorted(src_dir.glob("*.hip"))
        with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(8) as pool:
            parts = pool.map(lambda f: digest_file(f, src_dir / "../../include", defines, Path(tmp)), files)
            out.write_text(json.dumps({k: v for p in parts for k, v in p.items()}, indent=1, sort_keys=True))
        return 0
    old, new = (json.loads(Path(p).read_text()) for p in sys.argv[2:4])
    strip = lambda k: k.split("::", 1)[1]  # the file a kernel lives in may change
    new_by_name = {strip(k): k for k in new}
    left = set(new) - {new_by_name.get(strip(k)) for k in old}
    bad = 0
    for k, o in sorted(old.items()):
        nk = new_by_name.get(strip(k)) or next((c for c in sorted(left) if new[c] == o), None)
        left.discard(nk)
        same = nk is not None and new[nk] == o
        bad += not same
        print(f"{'identical' if same else 'DIFFERENT' if nk else 'MISSING  '} {o['bytes']:7d} B  v{o['vgpr_count']} a{o.get('agpr_count', 0)} s{o['sgpr_count']} "
              f"spill {o['vgpr_spill_count']}/{o['sgpr_spill_count']} scratch {o['private_segment_fixed_size']} lds {o['group_segment_fixed_size']}  {k}"
              + (f"  ->  {nk}" if nk and nk != k else ""))
    for k in sorted(left):
        print(f"NEW       {k}")
    print(f"{len(old)} kernels, {bad} not identical, {len(left)} new")
    return 1 if bad or left else 0


if __name__ == "__main__":
    sys.exit(main())
