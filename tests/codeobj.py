"""The product library as gfx950 device assembly, for the CPU tests that read a kernel's resource figures or instruction text.

``ihmr_hip.hip`` is compiled at most once per Python process, with the product's own flags (``hip.HIPCC_FLAGS`` without the two
that make a shared object), and the ``amdhsa.kernels`` metadata block is parsed once.  Callers check for ``hipcc`` themselves."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "ihmr_amd", "csrc")

_TEXT = _RECORDS = None


def assembly():
    """The whole assembly listing (about 10 MB of text)."""
    global _TEXT
    if _TEXT is None:
        from ihmr_amd import hip
        flags = [f for f in hip.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, "ihmr.s")
            cmd = ["hipcc"] + flags + [f"-I{os.path.join(ROOT, 'include')}", "--cuda-device-only", "-S", "-o", out, "ihmr_hip.hip"]
            r = subprocess.run(cmd, cwd=SRC, capture_output=True, text=True, timeout=900)
            assert r.returncode == 0, r.stderr[-3000:]
            with open(out) as fh:
                _TEXT = fh.read()
    return _TEXT


def records():
    """{mangled kernel name: {key: value}} with every integer key of the kernel's metadata record (a YAML list item at two
    spaces; `.name` sits in the middle of its sorted keys).  One record per `.amdhsa_kernel` directive, or the parser is wrong."""
    global _RECORDS
    if _RECORDS is None:
        text = assembly()
        recs = {}
        for rec in re.split(r"^  - (?=\.)", text[text.index("amdhsa.kernels:"):], flags=re.M)[1:]:
            name = re.search(r"^\s+\.name:\s+(\S+)", rec, flags=re.M).group(1)
            # the record's own keys: at four spaces, or -- the first one, behind the item's dash -- at none; an argument's lie deeper
            recs[name] = {k: int(v) for k, v in re.findall(r"^(?:\s{4})?\.(\w+):\s+(\d+)\s*$", rec, flags=re.M)}
            assert {"agpr_count", "sgpr_count", "vgpr_count", "private_segment_fixed_size"} <= set(recs[name]), (name, sorted(recs[name]))
        n = len(re.findall(r"^\s*\.amdhsa_kernel\s", text, flags=re.M))
        assert recs and len(recs) == n, (len(recs), n)
        _RECORDS = recs
    return _RECORDS


def matching(prefix):
    """{name: record} of the kernels whose mangled name starts with `prefix`."""
    return {n: r for n, r in records().items() if n.startswith(prefix)}


def kernel(prefix):
    """(name, record) of the one kernel whose mangled name starts with `prefix`."""
    hits = list(matching(prefix).items())
    assert len(hits) == 1, [n for n, _ in hits]
    return hits[0]


def body(name):
    """The lines of kernel `name` from its label to its first `s_endpgm`."""
    text = assembly()
    text = text[text.index(f"\n{name}:"):]
    return text[:text.index("s_endpgm")].splitlines()
