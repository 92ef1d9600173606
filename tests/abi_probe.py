"""One probe of include/shoulder_hip.h for the layout tests: what the header names (parsed from its text) and what a C compiler
makes of it (one program, generated from the header's constants and from the records and fields of shoulder_amd._lib.RECORDS,
compiled with gcc once per process)."""
import functools
import os
import re
import subprocess
import tempfile

from conftest import ROOT
from shoulder_amd import _lib

INCLUDE = os.path.join(ROOT, "include")


@functools.lru_cache(maxsize=None)
def header():
    """-> (records: C name -> field names in the header's order, for every `typedef struct sh_x { ... } sh_x;`;
           defines: the names of every `#define SH_X value`;  enums: the names of every enum member)"""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "shoulder_hip.h")).read(), flags=re.S)
    records = {}
    for cname, body in re.findall(r"typedef\s+struct\s+(sh_\w+)\s*\{(.*?)\}\s*\1\s*;", src, flags=re.S):
        decls = [d.split(None, 1)[1] for d in body.split(";") if d.strip()]                      # (the type is one word everywhere)
        records[cname] = [re.match(r"\s*(\w+)", part).group(1) for d in decls for part in d.split(",")]
    defines = re.findall(r"^#define[ \t]+(SH_[A-Z0-9_]+)[ \t]+\S", src, flags=re.M)
    enums = [m for body in re.findall(r"\benum\b[^{;]*\{(.*?)\}", src, flags=re.S) for m in re.findall(r"(?:^|,)\s*(SH_[A-Z0-9_]+)", body)]
    return records, defines, enums


@functools.lru_cache(maxsize=None)
def probe():
    """-> (sizes: C name -> sizeof;  offsets: C name -> {field: offsetof}, fields in the order of _lib.RECORDS;
           values: SH_X -> its value, for every #define and enum member of the header)"""
    _, defines, enums = header()
    lines = ['printf("V %s %%.17g\\n", (double)(%s));' % (n, n) for n in defines + enums]
    for cname, (cls, _) in _lib.RECORDS.items():
        lines.append('printf("S %s %%zu\\n", sizeof(%s));' % (cname, cname))
        lines += ['printf("O %s %s %%zu\\n", offsetof(%s, %s));' % (cname, n, cname, n) for n, _ in cls._fields_]
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "probe.c"), os.path.join(tmp, "probe")
        with open(src, "w") as f:
            f.write('#include <stdio.h>\n#include <stddef.h>\n#include "shoulder_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
        subprocess.check_call(["gcc", "-I", INCLUDE, "-o", exe, src])
        out = subprocess.check_output([exe], text=True)
    sizes, offsets, values = {}, {c: {} for c in _lib.RECORDS}, {}
    for kind, *w in (ln.split() for ln in out.splitlines()):
        if kind == "V":
            values[w[0]] = float(w[1])
        elif kind == "S":
            sizes[w[0]] = int(w[1])
        else:
            offsets[w[0]][w[1]] = int(w[2])
    return sizes, offsets, values
