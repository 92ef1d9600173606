#!/usr/bin/env python3
"""Kernel-by-kernel comparison of the device code of two builds of the library.
  python tools/device_code_diff.py OLD/libshoulder_hip.so NEW/libshoulder_hip.so
Every gfx950 code object of both libraries is extracted as tools/lib_census.py does and disassembled; the text is split per kernel
symbol, everything from `//` on a line (address and encoding) is dropped, and the kernels are compared by name, together with their
resource notes (registers, LDS, scratch).  Moving a kernel to another translation unit leaves all of this unchanged.
Exit status 0: same kernel names, each in exactly one code object, same text and resources."""
import collections, difflib, os, re, struct, subprocess, sys, tempfile
LLVM = "/opt/rocm/lib/llvm/bin"
NOTE_KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count")


def kernels(path):
    """{kernel: (text, resources)}, {kernel: number of code objects that define it}, number of code objects"""
    data = open(path, "rb").read()
    text, seen = {}, collections.Counter()
    offs = [m.start() for m in re.finditer(b"\x7fELF\x02\x01\x01\x40", data)]
    for o in offs:
        shoff = struct.unpack_from("<Q", data, o + 0x28)[0]
        shentsize, shnum = struct.unpack_from("<HH", data, o + 0x3A)
        with tempfile.NamedTemporaryFile(suffix=".co", delete=False) as f:
            f.write(data[o:o + shoff + shentsize * shnum]); name = f.name
        syms = subprocess.run([f"{LLVM}/llvm-readelf", "-s", "--wide", name], capture_output=True, text=True).stdout
        kd = {l.split()[-1][:-3] for l in syms.splitlines() if l.strip().endswith(".kd")}
        end = {}      # kernel -> first address behind it (what follows the last kernel of a section is padding, not code)
        for l in syms.splitlines():
            w = l.split()
            if len(w) >= 8 and w[3] == "FUNC" and w[-1] in kd:
                end[w[-1]] = int(w[1], 16) + int(w[2])
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", name], capture_output=True, text=True).stdout
        res = {}
        for blk in re.split(r"\n\s*- ", notes):
            m = re.search(r"\.name:\s+(\S+)", blk)
            if m:
                res[m.group(1).strip("'\"")] = tuple((k, (re.search(re.escape(k) + r":\s+(\S+)", blk) or [None, None])[1]) for k in NOTE_KEYS)
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", name], capture_output=True, text=True).stdout
        os.unlink(name)
        cur = None
        for ln in dis.splitlines():
            m = re.match(r"^[0-9a-f]* ?<([^>]+)>:$", ln)
            if m:
                cur = m.group(1) if m.group(1) in kd else (cur if cur and m.group(1).startswith(cur) else None)
                if cur and m.group(1) == cur:
                    seen[cur] += 1; text[cur] = []
                continue
            if cur:
                body, _, tail = ln.partition("//")
                body = body.rstrip()
                addr = re.match(r"\s*([0-9A-Fa-f]+):", tail)
                if body and body.strip() != "..." and not (addr and int(addr.group(1), 16) >= end.get(cur, 1 << 62)):
                    text[cur].append(body)
        for k in kd:
            text[k] = ("\n".join(text.get(k, [])), res.get(k))
    return text, seen, len(offs)


old, old_seen, n_old = kernels(sys.argv[1])
new, new_seen, n_new = kernels(sys.argv[2])
bad = 0
print(f"old: {n_old} code objects, {len(old)} kernels; new: {n_new} code objects, {len(new)} kernels")
for k in sorted(set(old) ^ set(new)):
    print("only in", "old" if k in old else "new", k); bad += 1
for k, n in sorted(new_seen.items()):
    if n != 1:
        print(f"{k}: defined in {n} code objects"); bad += 1
for k in sorted(set(old) & set(new)):
    if old[k][0] != new[k][0]:
        print("text differs:", k); bad += 1
        # the lines that differ: a moved constant table shows as pc-relative literals only, anything else as changed instructions
        for ln in difflib.unified_diff(old[k][0].splitlines(), new[k][0].splitlines(), "old", "new", lineterm="", n=1):
            print("   ", ln)
    elif not old[k][0]:
        print("no text found:", k); bad += 1
    if old[k][1] != new[k][1] or old[k][1] is None:
        print("resources differ:", k, old[k][1], new[k][1]); bad += 1
print("identical" if not bad else f"{bad} difference(s)")
sys.exit(1 if bad else 0)
