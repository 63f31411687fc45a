"""Per-kernel comparison of the gfx950 machine code of two builds of the library.

    python tools/kernel_diff.py OLD.so NEW.so [PATTERN]     (exit status 1 when a kernel differs)

For every kernel symbol of either library (those matching the regular expression PATTERN, when given) it
compares the instruction text -- addresses, encodings, local labels and pc-relative distances to globals
stripped, so a kernel that only moved to another code object or offset compares equal -- and the register, LDS and scratch sizes of the
metadata note, and prints `same`, `differs` (with the instruction counts and what differs), `only in OLD` or
`only in NEW`.  The code objects are extracted as tools/isa_audit.py does.
"""
from __future__ import annotations

import difflib
import re
import subprocess
import sys
from pathlib import Path

import isa_audit

META = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def _metadata(co: Path) -> dict:
    """kernel symbol -> {META key: value} from the code object's AMDGPU metadata note."""
    notes = subprocess.run([str(isa_audit.LLVM / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True,
                           check=True).stdout
    out, cur = {}, {}
    for line in notes.splitlines():
        m = re.match(r"\.(\w+):\s*(\S+)", line.strip().lstrip("- ").strip())
        if not m:
            continue
        key, val = m.groups()
        if key == "agpr_count":
            cur = {}  # (a kernel map starts with .agpr_count in sorted-key order)
        if key in META:
            cur[key] = int(val)
        elif key == "symbol":
            out[val.removesuffix(".kd")] = cur
    return out


def _instructions(co: Path, kernels) -> dict:
    """kernel symbol -> its instructions (text before the `//` comment), local labels dropped."""
    dis = subprocess.run([str(isa_audit.LLVM / "llvm-objdump"), "-d", "--mcpu=gfx950", str(co)], capture_output=True,
                         text=True, check=True).stdout
    out, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            if m.group(1) in kernels:
                cur = out.setdefault(m.group(1), [])
            elif not re.fullmatch(r"L\d+", m.group(1)):
                cur = None  # (a device function that is no kernel)
            continue
        s = line.split("//")[0].strip()
        if cur is None or not s or s == "...":  # ("...": the padding after a kernel's last instruction)
            continue
        # the literal added to s_getpc_b64's result is the distance to a global (the transfer tables), which
        # depends on where the linker put the kernel, not on its code
        if cur and cur[-1].startswith("s_getpc_b64") and s.startswith("s_add_u32"):
            s = re.sub(r"0x[0-9a-f]+$", "<pc-relative>", s)
        cur.append(s)
    return out


def kernels_of(lib: Path) -> dict:
    """kernel symbol -> (instructions, metadata) over every gfx950 code object of the library."""
    out = {}
    with isa_audit.code_objects(lib) as objs:
        for co in objs:
            meta = _metadata(co)
            for k, ins in _instructions(co, meta).items():
                out[k] = (ins, meta[k])
    return out


def main() -> int:
    if len(sys.argv) not in (3, 4):
        print(__doc__)
        return 2
    old, new = kernels_of(Path(sys.argv[1])), kernels_of(Path(sys.argv[2]))
    pat = re.compile(sys.argv[3]) if len(sys.argv) == 4 else None
    bad = 0
    for k in sorted(set(old) | set(new)):
        if pat and not pat.search(k):
            continue
        if k not in old or k not in new:
            print(f"only in {'NEW' if k in new else 'OLD'}  {k}")
            bad += 1
            continue
        (oi, om), (ni, nm) = old[k], new[k]
        if oi == ni and om == nm:
            print(f"same     {k}")
            continue
        bad += 1
        changed = sum(max(i2 - i1, j2 - j1)
                      for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, oi, ni, autojunk=False).get_opcodes()
                      if tag != "equal")
        what = [f"{len(oi)} -> {len(ni)} instructions, {changed} changed"]
        what += [f"{key} {om.get(key)} -> {nm.get(key)}" for key in META if om.get(key) != nm.get(key)]
        print(f"differs  {k}: " + "; ".join(what))
    print(f"{bad} kernel(s) differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
