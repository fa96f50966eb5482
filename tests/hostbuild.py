"""Stand-alone host programs of the CPU tests: the sanitizer flags, one builder, one runner, and the compiler's layout of the
header's structs.  Every program has its own `main` and is run directly; callers check for ``g++`` themselves."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-fno-fast-math"]
X86_V3 = ["-march=x86-64-v3"]        # extra of the drivers that have always been built for it


def build(source, out_dir, extra=()):
    """g++ with SAN (+ extra) of `source` -- a file name under tests/ or a path -- into `out_dir`; returns the program's path."""
    src = os.path.join(ROOT, "tests", str(source))
    exe = os.path.join(str(out_dir), os.path.splitext(os.path.basename(src))[0])
    subprocess.check_call(["g++"] + SAN + list(extra) + [src, "-o", exe])
    return exe


def run(exe, *args, ok=True):
    """Run the program with leak detection on.  A sanitizer report is a non-zero exit: asserts exit status 0 (ok=False: non-zero,
    for input the program must refuse) and returns the completed process."""
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert (r.returncode == 0) == ok, (r.returncode, r.stderr[-3000:])
    return r


def struct_layouts(structs):
    """{C struct name: [field names]} -> {C struct name: (sizeof, {field: offsetof})} as plain g++ lays out include/ihmr_hip.h."""
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "ihmr_hip.h"', "int main() {"]
    for s, fields in structs.items():
        lines.append(f'    printf("{s} %zu\\n", sizeof({s}));')
        lines += [f'    printf("{s}.{f} %zu\\n", offsetof({s}, {f}));' for f in fields]
    lines += ["    return 0;", "}", ""]
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "layout.cpp"), "w") as fh:
            fh.write("\n".join(lines))
        subprocess.check_call(["g++", "-I", os.path.join(ROOT, "include"), os.path.join(d, "layout.cpp"), "-o", os.path.join(d, "layout")])
        out = dict(l.split() for l in subprocess.check_output([os.path.join(d, "layout")], text=True).splitlines())
    return {s: (int(out[s]), {f: int(out[f"{s}.{f}"]) for f in fields}) for s, fields in structs.items()}
