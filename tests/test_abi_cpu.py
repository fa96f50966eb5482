"""include/ihmr_hip.h, the binding table ``hip.SIGNATURES`` and the ctypes mirrors of the header's structs agree: every prototype
argument by argument and in its return type, every struct in its size and in the offset of every field as g++ lays it out.  A
wrong ``c_int`` / ``c_void_p`` in a long call or a field added on one side only fails here, without a GPU."""
import ctypes as C
import os
import re
import shutil

import pytest

import hostbuild
from ihmr_amd import augment, hip

MIRRORS = dict(ihmr_opt_io=hip.OptIO, ihmr_opt_stage=hip.OptStage, ihmr_opt_weights=hip.OptWeights, ihmr_mlp_net=hip.MlpNet,
               ihmr_mlp_tables=hip.MlpTables, ihmr_mlp_stage=hip.MlpStage, ihmr_train_weights=hip.TrainWeights,
               ihmr_render_lights=hip.RenderLights, ihmr_sdf_options=hip.SdfOptions, ihmr_copy_seg=hip.CopySeg,
               ihmr_kernel_timer=hip.KernelTimer, ihmr_mano_arrays=hip.ManoArrays)
SCALARS = {C.c_int: "int", C.c_float: "float", C.c_size_t: "size_t", C.c_long: "long"}


def _header():
    """The header without comments and preprocessor lines."""
    with open(os.path.join(hostbuild.ROOT, "include", "ihmr_hip.h")) as fh:
        text = re.sub(r"/\*.*?\*/", " ", fh.read(), flags=re.S)
    return "\n".join(l for l in re.sub(r"//[^\n]*", " ", text).splitlines() if not l.lstrip().startswith("#"))


def _c_class(decl, is_parameter):
    """"int" | "float" | "size_t" | "long" | ("ptr", struct name or None) of a C parameter declaration or a return type."""
    decl = decl.strip()
    if "*" in decl:
        pointee = [t for t in decl[:decl.index("*")].split() if t != "const"]
        return ("ptr", pointee[0] if len(pointee) == 1 and pointee[0] in MIRRORS else None)
    tokens = [t for t in decl.split() if t != "const"]
    kind = tokens[:-1] if is_parameter and len(tokens) > 1 else tokens
    assert kind in (["int"], ["float"], ["size_t"], ["long"]), f"a type this test has no class for: {decl!r}"
    return kind[0]


def _prototypes():
    """{name: (return class, [parameter classes])} of every ihmr_* function the header declares."""
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(ihmr_\w+)\s*\(([^()]*)\)\s*;", _header()):
        assert name not in protos, name
        params = [] if params.strip() in ("", "void") else params.split(",")
        protos[name] = (_c_class(ret, False), [_c_class(p, True) for p in params])
    return protos


def _ctypes_class(t):
    if t in SCALARS:
        return SCALARS[t]
    if t in (C.c_void_p, C.c_char_p):
        return ("ptr", None)
    assert isinstance(t, type) and issubclass(t, C._Pointer), f"a ctypes type this test has no class for: {t!r}"
    return ("ptr", t._type_ if issubclass(t._type_, C.Structure) else None)


def _agree(c, py):
    """A pointer to a struct of the header is c_void_p or POINTER of that struct's mirror; any other pointer is no POINTER of a
    Structure; scalars are equal."""
    if isinstance(c, tuple) and isinstance(py, tuple):
        return py[1] is None or (c[1] is not None and py[1] is MIRRORS[c[1]])
    return c == py


def disagreements(signatures):
    protos, out = _prototypes(), []
    for name in sorted(set(protos) ^ set(signatures)):
        out.append(f"{name}: declared on one side only")
    for name in sorted(set(protos) & set(signatures)):
        (c_ret, c_args), (restype, argtypes) = protos[name], signatures[name]
        if not _agree(c_ret, _ctypes_class(restype)):
            out.append(f"{name}: returns {c_ret}, bound as {restype}")
        if len(c_args) != len(argtypes):
            out.append(f"{name}: {len(c_args)} parameters, {len(argtypes)} argtypes")
            continue
        out += [f"{name}: parameter {k} is {c}, bound as {t}" for k, (c, t) in enumerate(zip(c_args, argtypes)) if not _agree(c, _ctypes_class(t))]
    return out


def test_every_prototype_agrees_with_the_binding_table():
    protos = _prototypes()
    assert len(protos) == 77 and set(protos) == set(hip.SIGNATURES), set(protos) ^ set(hip.SIGNATURES)
    assert hip.EXPORTED_SYMBOLS == list(hip.SIGNATURES)
    assert protos["ihmr_version"] == (("ptr", None), []) and hip.SIGNATURES["ihmr_version"] == (C.c_char_p, [])
    assert protos["ihmr_conv_igemm"][1] == [("ptr", None)] * 5 + ["int"] * 16 + [("ptr", None), "size_t", ("ptr", None)]
    assert protos["ihmr_opt_run_stage"][1][2:6] == [("ptr", "ihmr_opt_io"), "int", ("ptr", "ihmr_opt_weights"), ("ptr", "ihmr_opt_stage")]
    assert disagreements(hip.SIGNATURES) == []


def test_the_comparison_reports_a_wrong_table():
    """The parser cannot pass by finding nothing: each mutation of a copy of the table is reported, at its function."""
    def mutated(name, change):
        restype, argtypes = hip.SIGNATURES[name]
        return dict(hip.SIGNATURES, **{name: change(restype, list(argtypes))})

    def swap(k):
        return lambda r, a: (r, a[:k] + [a[k + 1], a[k]] + a[k + 2:])
    cases = [("ihmr_conv_igemm", swap(4), 2),                                            # the last pointer and the first int of 24
             ("ihmr_adam_step", swap(4), 2),                                             # size_t and float
             ("ihmr_bn_train_forward", lambda r, a: (r, [a[0], C.c_int] + a[2:]), 1),    # long bound as int
             ("ihmr_opt_run_stage", lambda r, a: (r, a[:5] + [C.POINTER(hip.OptIO)] + a[6:]), 1),       # a pointer to another struct
             ("ihmr_sdf_collision", lambda r, a: (r, [C.POINTER(hip.SdfOptions)] + a[1:]), 1),          # a struct pointer for int32_t*
             ("ihmr_render_meshes", lambda r, a: (r, a[:-1]), 1),                        # arity
             ("ihmr_mano_workspace_bytes", lambda r, a: (C.c_int, a), 1),                # return type
             ("ihmr_version", lambda r, a: (C.c_int, a), 1)]
    for name, change, n in cases:
        found = disagreements(mutated(name, change))
        assert len(found) == n and all(f.startswith(name + ":") for f in found), (name, found)
    missing = {k: v for k, v in hip.SIGNATURES.items() if k != "ihmr_graph_launch"}
    assert disagreements(missing) == ["ihmr_graph_launch: declared on one side only"]
    assert disagreements(dict(hip.SIGNATURES, ihmr_debug_stamps=(C.c_int, []))) == ["ihmr_debug_stamps: declared on one side only"]


def _c_fields(struct):
    """The field names of `typedef struct NAME { ... } NAME;` in declaration order."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _header(), flags=re.S).group(1)
    names = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        names += [re.search(r"(\w+)\s*(\[[^\]]*\]\s*)*$", piece).group(1) for piece in decl.split(",")]
    return names


def test_every_mirror_names_the_fields_of_its_struct_in_order():
    for struct, mirror in MIRRORS.items():
        assert _c_fields(struct) == [f[0] for f in mirror._fields_], struct
    assert _c_fields("ihmr_aug_params") == list(augment.PARAMS_DTYPE.names)
    assert len(_c_fields("ihmr_opt_io")) == 31


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_every_mirror_has_the_size_and_the_offsets_of_its_struct():
    layouts = hostbuild.struct_layouts({s: _c_fields(s) for s in list(MIRRORS) + ["ihmr_aug_params"]})
    for struct, mirror in MIRRORS.items():
        size, offsets = layouts[struct]
        assert size == C.sizeof(mirror), (struct, size, C.sizeof(mirror))
        assert offsets == {name: getattr(mirror, name).offset for name, *_ in mirror._fields_}, struct
    size, offsets = layouts["ihmr_aug_params"]
    dt = augment.PARAMS_DTYPE
    assert size == dt.itemsize == 136 and offsets == {n: dt.fields[n][1] for n in dt.names}
    assert layouts["ihmr_opt_io"][1]["norm_batch"] == 24 * 8 and layouts["ihmr_opt_io"][0] == 24 * 8 + 7 * 4 + 4      # 24 pointers, 7 words, padding
