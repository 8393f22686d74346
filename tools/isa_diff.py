#!/usr/bin/env python3
"""Do two builds of libstn.so carry the same gfx950 device code?  The instrument of a refactor that claims to move kernels, not to change them.

Per kernel symbol of the gfx950 code objects (extracted as tests/test_isa_cpu.py extracts them) two things are compared:
  - the instruction stream as mnemonic + operands: addresses are dropped, and llvm-objdump prints branch targets as relative offsets, so a
    kernel that merely moved inside its code object, or to another one, compares equal;
  - the resource fields of its descriptor as the code object's metadata note states them: VGPR, AGPR and SGPR counts, LDS bytes, scratch bytes.
Prints the symbols present on one side only and the kernels that differ (with the first differing instruction).

usage: tools/isa_diff.py [--map OLD=NEW ...] old/libstn.so new/libstn.so      exit code 1 when anything differs.  Needs no GPU.

--map OLD=NEW pairs a renamed kernel: the one symbol present only in the old build whose name contains OLD with the one present only in
the new build whose name contains NEW.  A pair is compared like a kept symbol, and its instruction counts and resource fields are
printed for both sides whether they differ or not.
"""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_hazards import OBJDUMP, parse  # noqa: E402

READELF = os.path.join(os.path.dirname(OBJDUMP), "llvm-readelf")
RESOURCES = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def resources(code_object):
    """{kernel symbol: {field: value}} from the NT_AMDGPU_METADATA note"""
    note = subprocess.run([READELF, "--notes", code_object], check=True, capture_output=True, text=True).stdout
    out = {}
    for block in re.split(r"^  - (?=\.)", note, flags=re.M)[1:]:  # one list item of amdhsa.kernels each
        name = re.search(r"^\s+\.name:\s+(\S+)", block, flags=re.M)
        if name:
            out[name.group(1)] = {f: int(m.group(1)) for f in RESOURCES for m in [re.search(rf"^\s*\.{f}:\s+(\d+)", block, flags=re.M)] if m}
    return out


def load(lib):
    """{symbol: ([(mnemonic, operands)], resource fields or None for a device function that is no kernel)}"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        copy = os.path.join(tmp, "libstn.so")
        shutil.copy(lib, copy)
        subprocess.run([OBJDUMP, "--offloading", copy], check=True, capture_output=True, cwd=tmp)  # writes <copy>.N.<triple>
        objs = sorted(glob.glob(copy + ".*gfx950"))
        if not objs:
            raise SystemExit("no gfx950 code object in " + lib)
        for co in objs:
            res = resources(co)
            for name, ins in parse(co).items():
                if name in out:
                    raise SystemExit(f"{lib}: {name} is defined in two code objects")
                out[name] = ([(op, args) for _, op, args in ins], res.get(name))
    return out


def pair(old, new, maps):
    """the symbols of `new` that a --map pairs with a symbol of `old` take that symbol's name; returns {old name: new name}"""
    only_old, only_new = set(old) - set(new), set(new) - set(old)
    paired = {}
    for m in maps:
        a, _, b = m.partition("=")
        sa, sb = [n for n in only_old if a in n], [n for n in only_new if b in n]
        if not (a and b and len(sa) == 1 and len(sb) == 1):
            raise SystemExit(f"--map {m}: {len(sa)} old and {len(sb)} new unpaired symbols match, need one of each")
        paired[sa[0]] = sb[0]
        new[sa[0]] = new.pop(sb[0])
        only_old.discard(sa[0])
        only_new.discard(sb[0])
    return paired


def main():
    args, maps = sys.argv[1:], []
    while args and args[0] == "--map" and len(args) > 1:
        maps.append(args[1])
        args = args[2:]
    if len(args) != 2:
        raise SystemExit(__doc__)
    old, new = load(args[0]), load(args[1])
    paired = pair(old, new, maps)
    bad = 0
    for side, only in (("old", sorted(set(old) - set(new))), ("new", sorted(set(new) - set(old)))):
        for name in only:
            print(f"only in {side}: {name}")
        bad += len(only)
    for name in sorted(set(old) & set(new)):
        (ia, ra), (ib, rb) = old[name], new[name]
        if name in paired:
            print(f"paired: {name}\n    with {paired[name]}\n    old {len(ia)} instructions {ra}\n    new {len(ib)} instructions {rb}")
        if ra != rb:
            print(f"resources differ: {name}\n    old {ra}\n    new {rb}")
        if ia != ib:
            at = next((i for i, (x, y) in enumerate(zip(ia, ib)) if x != y), min(len(ia), len(ib)))
            show = lambda s: " ".join(s[at]) if at < len(s) else "(end)"  # noqa: E731
            print(f"instructions differ: {name}\n    {len(ia)} against {len(ib)} instructions, first difference at #{at}: {show(ia)}  |  {show(ib)}")
        bad += ra != rb or ia != ib
    kernels = sum(1 for _, r in new.values() if r is not None)
    print(f"{len(new)} symbols ({kernels} kernels) in {args[1]}: {bad} missing or different against {args[0]}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
