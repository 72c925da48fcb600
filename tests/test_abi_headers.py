"""The whole seam between the headers under include/ and mbexwn_vocoder_amd/abi.py, on the CPU and without a compute call:
every function of every header (names, order, one header each, exported), every parameter and return type of abi.TABLE
against its prototype, every field of every ctypes structure against the C compiler's layout.  Each comparison is also fed
doctored data of the test's own, so that it is seen to fail when the two sides disagree."""
import collections
import ctypes
import os
import subprocess

import pytest

import c_headers
from mbexwn_vocoder_amd import abi
from mbexwn_vocoder_amd.build import LIB_PATH, build_library

SCALARS = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "size_t": ctypes.c_size_t}
RESTYPES = {"mbx_status": ctypes.c_int32, "size_t": ctypes.c_size_t, "const char *": ctypes.c_char_p}
# what a typed pointer of the table may point to, by the C base type; the other base types are bound as c_void_p only
POINTEES = dict({"float": ctypes.c_float, "double": ctypes.c_double, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64,
                 "char": ctypes.c_char}, **{st.__name__: st for st in abi.STRUCTS})
OPAQUE = {"void", "mbx_handle", "mbx_stream_state", "uint64_t", "uint16_t", "uint8_t", "int16_t"}


# ------------------------------------------------------------------------------------------------------------------------
# every function of every header
# ------------------------------------------------------------------------------------------------------------------------
def declared():
    return {header: c_headers.prototypes(c_headers.read_code(header)) for header in c_headers.header_names()}


def name_mismatches(protos, table):
    """protos: {header: [(name, return type, parameter list)]}; table: abi.TABLE's shape.  [] when the names agree header by
    header and in order and no name is declared twice."""
    out = []
    if sorted(protos) != sorted(table):
        out.append(f"headers {sorted(protos)} != table {sorted(table)}")
    for header in sorted(set(protos) & set(table)):
        names, bound = [pp[0] for pp in protos[header]], [row[0] for row in table[header]]
        if names != bound:
            out.append(f"{header}: declares {names}, the table has {bound}")
    for names in ([pp[0] for rows in protos.values() for pp in rows], [row[0] for rows in table.values() for row in rows]):
        out += [f"{name} appears {count} times" for name, count in collections.Counter(names).items() if count != 1]
    return out


def test_every_function_of_every_header_is_in_the_table_and_exported():
    protos = declared()
    assert name_mismatches(protos, abi.TABLE) == []
    assert [abi.symbols(header) for header in abi.TABLE] == [[row[0] for row in rows] for rows in abi.TABLE.values()]
    assert abi.all_symbols() == [name for header in abi.TABLE for name in abi.symbols(header)]
    names = abi.all_symbols()
    assert len(names) == len(set(names)) >= 42 and {"mbx_forward", "mbx_create", "mbxc_decode_f0"} <= set(names)
    build_library()
    assert os.path.exists(LIB_PATH)
    lib = abi.load_library()
    for name in names:
        assert hasattr(lib, name), f"{name} is declared and bound but not exported"
        assert getattr(lib, name).argtypes is not None, name


def test_the_name_comparison_bites():
    code = "mbx_status mbxz_one(int32_t a);\nconst char *mbxz_two(void);\n"
    protos = {"z.h": c_headers.prototypes(code)}
    assert protos == {"z.h": [("mbxz_one", "mbx_status", "int32_t a"), ("mbxz_two", "const char *", "void")]}
    good = {"z.h": [("mbxz_one", ctypes.c_int32, [ctypes.c_int32]), ("mbxz_two", ctypes.c_char_p, [])]}
    assert name_mismatches(protos, good) == []
    assert name_mismatches(protos, {"z.h": good["z.h"][::-1]})                   # the header's order
    assert name_mismatches(protos, {"z.h": good["z.h"][:1]})                     # declared, not bound
    assert name_mismatches({"z.h": protos["z.h"][:1]}, good)                     # bound, not declared
    assert name_mismatches(protos, dict(good, **{"y.h": []}))                    # a header the table has and include/ has not
    twice = {"z.h": protos["z.h"], "y.h": protos["z.h"][:1]}
    assert any("mbxz_one appears 2 times" in line for line in name_mismatches(twice, dict(good, **{"y.h": good["z.h"][:1]})))
    # a declaration the parser cannot read is an error, never a gap: a function pointer, a return type on the line above
    for bad in ("mbx_status mbxz_three(void (*fn)(int));", "mbx_status\nmbxz_three(int32_t a);", "mbx_status mbxz_three(int32_t a) {}"):
        with pytest.raises(ValueError, match="unreadable"):
            c_headers.prototypes(code + bad)
    # comments do not declare anything
    assert c_headers.read_code("mbexwn_audio.h").count("mbxa_resample_poly") == 1


# ------------------------------------------------------------------------------------------------------------------------
# every parameter
# ------------------------------------------------------------------------------------------------------------------------
def parameter_mismatch(base, depth, bound):
    """None when the ctypes type `bound` binds a C parameter of `depth` stars on `base`; else what is wrong."""
    if depth == 0:
        if base not in SCALARS:
            return f"cannot classify the scalar type {base}"
        return None if bound is SCALARS[base] else f"{base} bound as {bound.__name__}"
    if base not in POINTEES and base not in OPAQUE:
        return f"cannot classify a pointer to {base}"
    if bound is ctypes.c_void_p:
        return None
    if bound is ctypes.c_char_p:
        return None if (base, depth) == ("char", 1) else f"{base} {'*' * depth} bound as c_char_p"
    if not (isinstance(bound, type) and issubclass(bound, ctypes._Pointer)):
        return f"{base} {'*' * depth} bound as {getattr(bound, '__name__', bound)}, which is no pointer"
    want = ctypes.c_void_p if depth == 2 else POINTEES.get(base) if depth == 1 else None
    return None if want is not None and bound._type_ is want else f"{base} {'*' * depth} bound as a pointer to {bound._type_.__name__}"


def binding_mismatches(protos, table):
    out = []
    for header, rows in table.items():
        by_name = {pp[0]: pp for pp in protos[header]}
        for name, restype, argtypes in rows:
            _, ret, plist = by_name[name]
            if ret not in RESTYPES:
                out.append(f"{name}: cannot classify the return type {ret}")
            elif restype is not RESTYPES[ret]:
                out.append(f"{name}: returns {ret}, restype {getattr(restype, '__name__', restype)}")
            params = c_headers.parameters(plist)
            if len(params) != len(argtypes):
                out.append(f"{name}: {len(params)} parameters, {len(argtypes)} argtypes")
                continue
            for (base, depth, pname), bound in zip(params, argtypes):
                why = parameter_mismatch(base, depth, bound)
                if why:
                    out.append(f"{name}({pname}): {why}")
    return out


def test_every_parameter_and_return_type_matches_its_prototype():
    protos = declared()
    assert binding_mismatches(protos, abi.TABLE) == []
    checked = sum(len(row[2]) for rows in abi.TABLE.values() for row in rows)
    assert checked == sum(len(c_headers.parameters(pp[2])) for rows in protos.values() for pp in rows) > 0
    # the typed pointers the table has are compared by pointee: the ones the wrappers rely on
    table = {row[0]: row for rows in abi.TABLE.values() for row in rows}
    assert table["mbx_create"][2][0] is ctypes.POINTER(abi.mbx_config) and table["mbx_stage"][2][3] is ctypes.POINTER(ctypes.c_int64)
    assert table["mbxc_f0_candidates"][2][12] is table["mbxc_f0_candidates"][2][13] is ctypes.POINTER(ctypes.c_float)
    assert table["mbx_workspace_size"][1] is ctypes.c_size_t and table["mbx_last_error"][1] is ctypes.c_char_p


def test_the_parameter_comparison_bites():
    i32, i64, f32, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    P = ctypes.POINTER
    code = ("mbx_status mbxz_run(const mbx_config *config, const float *x, int64_t stride, float eps, const int64_t *desc,\n"
            "                    mbx_handle **out, const char *name, size_t bytes, void *hip_stream);\n"
            "size_t mbxz_size(const mbx_handle *handle);\n")
    protos = {"z.h": c_headers.prototypes(code)}
    assert c_headers.parameters(protos["z.h"][0][2])[:3] == [("mbx_config", 1, "config"), ("float", 1, "x"), ("int64_t", 0, "stride")]
    good = [P(abi.mbx_config), vp, i64, f32, P(i64), P(vp), ctypes.c_char_p, ctypes.c_size_t, vp]

    def lines(argtypes=good, restype=i32, size_restype=ctypes.c_size_t, source=protos):
        return binding_mismatches(source, {"z.h": [("mbxz_run", restype, argtypes), ("mbxz_size", size_restype, [vp])]})

    assert lines() == [] and lines([vp, P(f32), i64, f32, vp, vp, vp, ctypes.c_size_t, vp]) == []

    def swapped(index, bound):
        return lines(good[:index] + [bound] + good[index + 1:])

    assert "int64_t bound as c_int" in swapped(2, i32)[0]                        # a stride that would truncate
    assert "float bound as c_int" in swapped(3, i32)[0]                          # a float passed as garbage
    assert "size_t bound as c_int" in swapped(7, i32)[0]
    assert "no pointer" in swapped(1, i32)[0] and "no pointer" in swapped(8, i64)[0]
    assert "pointer to c_int" in swapped(4, P(i32))[0]                           # the pointee of a typed pointer
    assert "pointer to mbx_tensor" in swapped(0, P(abi.mbx_tensor))[0]
    assert "pointer to c_float" in swapped(5, P(f32))[0] and "bound as c_char_p" in swapped(1, ctypes.c_char_p)[0]
    assert "pointer to" in swapped(8, P(i32))[0]                                 # void * takes no typed pointer
    assert "8 argtypes" in lines(good[:-1])[0] and "10 argtypes" in lines(good + [vp])[0]
    assert "returns mbx_status" in lines(restype=ctypes.c_size_t)[0] and "returns size_t" in lines(size_restype=i32)[0]
    assert "returns mbx_status" in lines(restype=None)[0]
    for decl, word in (("unsigned flags", "cannot classify the scalar type unsigned"), ("double gain", "scalar type double"),
                       ("const mbx_thing *thing", "cannot classify a pointer to mbx_thing")):
        other = {"z.h": c_headers.prototypes(code.replace("float eps", decl))}
        assert word in lines(source=other)[0], decl
    other = {"z.h": c_headers.prototypes(code.replace("size_t mbxz_size", "int mbxz_size"))}
    assert "cannot classify the return type int" in lines(source=other)[0]
    with pytest.raises(ValueError, match="unreadable parameter"):
        c_headers.parameters("const float x[4]")


# ------------------------------------------------------------------------------------------------------------------------
# every field of every struct
# ------------------------------------------------------------------------------------------------------------------------
KIND = ("_Generic(({x}), float: 'f', double: 'd', char: 'c', int32_t: 'i', int64_t: 'l', mbx_subnet_op: 's', "
        "const char *: 'p', char *: 'p', const float *: 'p', float *: 'p', const int32_t *: 'p', int32_t *: 'p', "
        "const void *: 'p', void *: 'p', const mbx_stream_state *: 'p', mbx_stream_state *: 'p', default: '?')")
SIMPLE = {ctypes.c_float: "f", ctypes.c_double: "d", ctypes.c_char: "c", ctypes.c_int32: "i", ctypes.c_int64: "l"}


def field_kind(ctype):
    if issubclass(ctype, ctypes.Structure):
        return "s"
    if ctype in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(ctype, ctypes._Pointer):
        return "p"
    return SIMPLE[ctype]


def layout_program(structs):
    """(C source, the records ctypes expects of it): "sizeof" per struct, then offsetof, sizeof and the type code of each
    field -- of its element [0] for an array.  The field names come from _fields_: a renamed field does not compile."""
    lines, want = [], []
    for st in structs:
        name = st.__name__
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        want.append(f"{name} {ctypes.sizeof(st)}")
        for field, ctype in st._fields_:
            array = issubclass(ctype, ctypes.Array)
            member = f"(({name} *)0)->{field}"
            code = KIND.format(x=member + ("[0]" if array else ""))
            lines.append(f'printf("{name}.{field} %zu %zu %c\\n", offsetof({name}, {field}), sizeof({member}), {code});')
            want.append(f"{name}.{field} {getattr(st, field).offset} {ctypes.sizeof(ctype)} {field_kind(ctype._type_ if array else ctype)}")
    source = ('#include <stdio.h>\n#include <stddef.h>\n#include "mbexwn.h"\nint main(void) {\n' + "\n".join(lines)
              + "\nreturn 0;\n}\n")
    return source, want


def compiled_layout(tmp_path, structs, tag="layout"):
    source, want = layout_program(structs)
    src, exe = tmp_path / f"{tag}.c", tmp_path / tag
    src.write_text(source)
    res = subprocess.run(["gcc", "-std=c11", "-I", c_headers.INCLUDE, str(src), "-o", str(exe)], capture_output=True, text=True)
    if res.returncode != 0:
        return None, want, res.stderr
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines(), want, ""


def test_every_field_of_every_struct_has_the_c_layout(tmp_path):
    assert [st.__name__ for st in abi.STRUCTS] == ["mbx_subnet_op", "mbx_config", "mbx_tensor", "mbx_conv_form_info",
                                                   "mbx_kernel_report_info", "mbx_plan_info", "mbx_forward_options"]
    got, want, err = compiled_layout(tmp_path, abi.STRUCTS)
    assert got is not None, err
    assert len(want) == len(abi.STRUCTS) + sum(len(st._fields_) for st in abi.STRUCTS) >= 159
    for have, expect in zip(got, want):
        assert have == expect                                            # record by record: the first one off is named
    assert len(got) == len(want) and not [line for line in got if line.endswith("?")]


def test_the_layout_comparison_bites(tmp_path):
    def doctored(struct, change):
        return type(struct.__name__, (ctypes.Structure,), {"_fields_": [change.get(ff[0], ff) for ff in struct._fields_]})

    def differing(struct, change, tag):
        got, want, err = compiled_layout(tmp_path, [doctored(struct, change)], tag)
        assert got is not None, err
        return [(have, expect) for have, expect in zip(got, want) if have != expect]

    assert differing(abi.mbx_tensor, {}, "same") == []
    # a float mirrored as an int of the same size: only the type code tells
    assert differing(abi.mbx_subnet_op, {"alpha": ("alpha", ctypes.c_int32)}, "kind") == [("mbx_subnet_op.alpha 36 4 f", "mbx_subnet_op.alpha 36 4 i")]
    # a pointer mirrored as a 64-bit integer, an int64 array as a double array
    assert differing(abi.mbx_forward_options, {"f0": ("f0", ctypes.c_int64)}, "ptr") == [("mbx_forward_options.f0 8 8 p", "mbx_forward_options.f0 8 8 l")]
    assert [pair[0] for pair in differing(abi.mbx_tensor, {"shape": ("shape", ctypes.c_double * 4)}, "elem")] == ["mbx_tensor.shape 24 32 l"]
    # a width: every later offset and the size move
    assert len(differing(abi.mbx_subnet_op, {"kind": ("kind", ctypes.c_int64)}, "width")) == 1 + len(abi.mbx_subnet_op._fields_)
    # an array length, a dropped last field
    assert differing(abi.mbx_plan_info, {"gate_kernel": ("gate_kernel", ctypes.c_int32 * 63)}, "length")
    short = type("mbx_plan_info", (ctypes.Structure,), {"_fields_": abi.mbx_plan_info._fields_[:-1]})
    got, want, _ = compiled_layout(tmp_path, [short], "short")
    assert got[0] != want[0] and got[1:] == want[1:]
    # a renamed field does not compile
    got, _, err = compiled_layout(tmp_path, [doctored(abi.mbx_tensor, {"ndim": ("rank", ctypes.c_int32)})], "renamed")
    assert got is None and "rank" in err
