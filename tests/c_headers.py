"""The function declarations of the public headers under include/, read with regular expressions (the headers are plain C
with one declaration style: the return type at the start of a line, no function pointers, /* */ comments)."""
import os
import re

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
_PROTOTYPE = re.compile(r"^((?:const[ \t]+)?\w+[ \t]*\*?)[ \t]*\b(mbx[a-z]?_\w+)\s*\(([^;{()]*)\)\s*;", re.M)
_PARAMETER = re.compile(r"(?:const\s+)?(\w+)\s*((?:\*\s*)*)(\w+)")


def header_names():
    return sorted(name for name in os.listdir(INCLUDE) if name.endswith(".h"))


def read_code(header):
    """The text of include/<header> with its comments taken out."""
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(INCLUDE, header)).read(), flags=re.S)


def prototypes(code):
    """[(name, return type, parameter list)] in the order of declaration, white space normalised.  Every lower-case mbx*_ name
    in front of a parenthesis must be one of them: a declaration in a style this parser does not read is an error, not a gap."""
    found = [(mm.group(2), " ".join(mm.group(1).split()), " ".join(mm.group(3).split())) for mm in _PROTOTYPE.finditer(code)]
    called = re.findall(r"\b(mbx[a-z]?_[a-z0-9_]+)\s*\(", code)
    if called != [name for name, _, _ in found]:
        raise ValueError(f"unreadable declaration among {sorted(set(called) ^ {name for name, _, _ in found}) or called}")
    return found


def parameters(parameter_list):
    """[(base type, pointer depth, name)] of "const float *x, int32_t n"; "void" is no parameter."""
    out = []
    for decl in ([] if parameter_list.strip() in ("", "void") else parameter_list.split(",")):
        mm = _PARAMETER.fullmatch(decl.strip())
        if not mm:
            raise ValueError(f"unreadable parameter {decl.strip()!r}")
        out.append((mm.group(1), mm.group(2).count("*"), mm.group(3)))
    return out
