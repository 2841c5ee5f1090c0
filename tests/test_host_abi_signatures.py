"""The ctypes tables of fullsubnet_plus_amd._lib against the prototypes of include/*.h, TYPE BY TYPE (the per-header tests compare names).

A stride typed c_int32 where the header says int64_t, or a parameter left out, still loads and still runs - with garbage in a register
that becomes a pointer or a size on the device.  So every prototype of every header in _lib.HEADER_TABLES is parsed here and reduced,
like its table entry, to width classes: ptr, i32, i64, f64, size_t, void.  No GPU and no library: text against tables."""
import ctypes
import glob
import os
import re

import pytest

from fullsubnet_plus_amd import _lib

INCLUDE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include")
SCALARS = {"int": "i32", "int32_t": "i32", "int64_t": "i64", "double": "f64", "size_t": "size_t", "void": "void"}
PROTOTYPE = re.compile(r"(?:\A|(?<=[;{}]))\s*([A-Za-z_][\w\s\*]*?)\b(fsnp_\w+)\s*\(([^()]*)\)\s*;")


def strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return re.sub(r"^\s*#[^\n]*", " ", text, flags=re.M)          # preprocessor lines


def c_class(decl):
    """`const int64_t strides[3]` -> "ptr", `int32_t batch` -> "i32", `void` -> "void": the width class of a return type or parameter."""
    if "*" in decl or "[" in decl:
        return "ptr"
    words = [w for w in re.findall(r"\w+", decl) if w not in ("const", "extern", "struct")]
    if not words or words[0] not in SCALARS:
        raise ValueError(f"no width class for the C declaration {decl!r}")
    return SCALARS[words[0]]


def parse_prototypes(text):
    """-> {name: (return class, [parameter classes])} of every fsnp_* prototype in a header's text."""
    out = {}
    for ret, name, params in PROTOTYPE.findall(strip_comments(text)):
        params = [p.strip() for p in params.split(",")]
        if params in ([""], ["void"]):
            params = []
        assert name not in out, f"{name} is declared twice"
        out[name] = (c_class(ret), [c_class(p) for p in params])
    return out


def ctypes_class(t):
    if t is None:
        return "void"
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, (ctypes._Pointer, ctypes.Array)):
        return "ptr"
    # (size_t first: where it has the width of int64_t it is still another ctypes class, c_ulong against c_long)
    for ct, cls in ((ctypes.c_size_t, "size_t"), (ctypes.c_int32, "i32"), (ctypes.c_int64, "i64"), (ctypes.c_double, "f64")):
        if t is ct:
            return cls
    raise ValueError(f"no width class for the ctypes type {t!r}")


def table_classes(table):
    return {name: (ctypes_class(res), [ctypes_class(a) for a in args]) for name, (res, args) in table.items()}


def mismatches(declared, bound):
    """-> one line per difference between parse_prototypes' and table_classes' view of the same names."""
    out = [f"{n}: declared, not bound" for n in sorted(set(declared) - set(bound))]
    out += [f"{n}: bound, not declared" for n in sorted(set(bound) - set(declared))]
    for n in sorted(set(declared) & set(bound)):
        (dres, dargs), (bres, bargs) = declared[n], bound[n]
        if dres != bres:
            out.append(f"{n}: returns {dres}, restype is {bres}")
        if len(dargs) != len(bargs):
            out.append(f"{n}: {len(dargs)} parameters, {len(bargs)} argtypes")
        out += [f"{n}: parameter {i} is {d}, argtypes[{i}] is {b}" for i, (d, b) in enumerate(zip(dargs, bargs)) if d != b]
    return out


def header_text(name):
    with open(os.path.join(INCLUDE, name)) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------ the parser itself, on synthetic text
SYNTHETIC = """
/* int fsnp_in_a_comment(int32_t a); */
#define FSNP_MACRO(x) fsnp_not_a_prototype(x);
typedef struct fsnp_handle fsnp_handle;
int fsnp_push(fsnp_handle* h, const float* x, int64_t stride, const int64_t strides[3],   // int fsnp_line_comment(void);
              int32_t n, double scale, void* hip_stream);
size_t fsnp_bytes(const fsnp_handle* h, int batch);
const char* fsnp_text(void);
void fsnp_free(fsnp_handle* h);
int64_t fsnp_count(const void* const* ptrs);
"""
c_i32, c_i64, c_vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
SYNTHETIC_TABLE = {
    "fsnp_push": (c_i32, [c_vp, c_vp, c_i64, ctypes.POINTER(c_i64 * 3), c_i32, ctypes.c_double, c_vp]),
    "fsnp_bytes": (ctypes.c_size_t, [c_vp, c_i32]),
    "fsnp_text": (ctypes.c_char_p, []),
    "fsnp_free": (None, [c_vp]),
    "fsnp_count": (c_i64, [ctypes.POINTER(c_vp)]),
}


def test_parser_reads_the_synthetic_header():
    declared = parse_prototypes(SYNTHETIC)
    assert declared == {"fsnp_push": ("i32", ["ptr", "ptr", "i64", "ptr", "i32", "f64", "ptr"]), "fsnp_bytes": ("size_t", ["ptr", "i32"]),
                        "fsnp_text": ("ptr", []), "fsnp_free": ("void", ["ptr"]), "fsnp_count": ("i64", ["ptr"])}
    assert mismatches(declared, table_classes(SYNTHETIC_TABLE)) == []
    with pytest.raises(ValueError, match="no width class"):
        parse_prototypes("int fsnp_f(unsigned long n);")
    with pytest.raises(ValueError, match="no width class"):
        ctypes_class(ctypes.c_float)


def _push(**change):
    res, args = SYNTHETIC_TABLE["fsnp_push"]
    args = list(args)
    for k, v in change.items():
        if k == "res":
            res = v
        elif k == "drop":
            del args[v]
        elif k == "add":
            args.append(v)
        else:
            args[int(k[1:])] = v
    return dict(SYNTHETIC_TABLE, fsnp_push=(res, args))


@pytest.mark.parametrize("table,expected", [
    (_push(a2=c_i32, a4=c_i64), ["fsnp_push: parameter 2 is i64, argtypes[2] is i32", "fsnp_push: parameter 4 is i32, argtypes[4] is i64"]),
    (_push(drop=4), None),
    (_push(add=c_i32), ["fsnp_push: 7 parameters, 8 argtypes"]),
    (_push(res=c_i64), ["fsnp_push: returns i32, restype is i64"]),
    (_push(a3=c_i64), ["fsnp_push: parameter 3 is ptr, argtypes[3] is i64"]),
], ids=["i32_i64_swapped", "dropped_parameter", "added_parameter", "wrong_return_type", "array_as_integer"])
def test_parser_flags_a_wrong_table(table, expected):
    found = mismatches(parse_prototypes(SYNTHETIC), table_classes(table))
    if expected is None:          # the parameters behind the dropped one shift too: the count is what must be named
        assert "fsnp_push: 7 parameters, 6 argtypes" in found
    else:
        assert found == expected


def test_names_in_one_table_only_are_flagged():
    declared = parse_prototypes(SYNTHETIC)
    bound = table_classes({k: v for k, v in SYNTHETIC_TABLE.items() if k != "fsnp_free"})
    assert mismatches(declared, bound) == ["fsnp_free: declared, not bound"]
    assert mismatches({k: v for k, v in declared.items() if k != "fsnp_text"}, table_classes(SYNTHETIC_TABLE)) == ["fsnp_text: bound, not declared"]


# ------------------------------------------------------------------------------------------------ the real headers against the real tables
def test_registry_names_every_header_and_every_table():
    on_disk = {os.path.basename(p) for p in glob.glob(os.path.join(INCLUDE, "*.h"))}
    assert on_disk == set(_lib.HEADER_TABLES)
    tables = [v for k, v in vars(_lib).items() if k.endswith("SYMBOLS") and isinstance(v, dict)]
    assert len(tables) == 11 and all(any(t is r for r in _lib.HEADER_TABLES.values()) for t in tables)
    assert _lib.HEADER_TABLES["fsnp.h"] is _lib.HEADER_TABLES["fsnp_debug.h"] is _lib.SYMBOLS
    assert len(_lib.all_symbols()) == sum(len(t) for t in tables) == 134


def test_a_name_in_two_tables_is_refused():
    one, two = {"fsnp_a": (None, [])}, {"fsnp_b": (None, []), "fsnp_a": (None, [])}
    assert set(_lib.all_symbols({"a.h": one, "a_debug.h": one, "b.h": {"fsnp_b": (None, [])}})) == {"fsnp_a", "fsnp_b"}
    with pytest.raises(RuntimeError, match=r"fsnp_a.*b\.h"):
        _lib.all_symbols({"a.h": one, "b.h": two})


def test_every_prototype_matches_its_table_type_by_type():
    """Every prototype of include/*.h is bound in the table registered for its header with the same width classes, position by position,
    and every table entry is declared in (one of) its header(s)."""
    by_table, total = {}, 0
    for header, table in _lib.HEADER_TABLES.items():
        declared = parse_prototypes(header_text(header))
        assert declared, header
        total += len(declared)
        entry = by_table.setdefault(id(table), (table, {}, []))
        assert not set(entry[1]) & set(declared), f"{header}: declared in another header of the same table too"
        entry[1].update(declared)
        entry[2].append(header)
    assert total == 134
    wrong = []
    for table, declared, headers in by_table.values():
        wrong += [f"{'+'.join(headers)}: {line}" for line in mismatches(declared, table_classes(table))]
    assert not wrong, "\n".join(wrong)


def test_fsnp_config_fields_match_the_struct():
    """names, order and array lengths of struct fsnp_config against FsnpConfig._fields_ (every field is an int32_t)."""
    body = re.search(r"typedef struct fsnp_config \{(.*?)\} fsnp_config;", strip_comments(header_text("fsnp.h")), flags=re.S).group(1)
    declared = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.fullmatch(r"int32_t\s+(\w+)\s*(?:\[\s*(\d+)\s*\])?", decl)
        assert m, decl
        declared.append((m.group(1), int(m.group(2)) if m.group(2) else None))
    bound = []
    for name, t in _lib.FsnpConfig._fields_:
        length = t._length_ if issubclass(t, ctypes.Array) else None
        assert (t._type_ if length else t) is ctypes.c_int32, name
        bound.append((name, length))
    assert declared == bound and len(bound) == 17
    assert ctypes.sizeof(_lib.FsnpConfig) == 76 == 4 * sum(n or 1 for _, n in bound)
