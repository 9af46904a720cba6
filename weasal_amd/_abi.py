"""The ctypes view of a C header: prototypes, struct layouts and integer constants, read from the header's text.

Pure functions, no device, no library.  Only `ws_*` names are read.  A declaration ends in `;`; a function definition
(a body in braces) is not one.  Types: int, [u]int{8,16,32,64}_t, float, double by value; `char*` is c_char_p; every other
pointer (`T*`, `T**`, `T name[]`) is c_void_p; a `void` return is None.  Anything else raises AbiError naming the
declaration: nothing is guessed and nothing is skipped.
"""
import collections
import ctypes as C
import re

Abi = collections.namedtuple("Abi", "prototypes structs constants")

_SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double,
            "int8_t": C.c_int8, "int16_t": C.c_int16, "int32_t": C.c_int32, "int64_t": C.c_int64,
            "uint8_t": C.c_uint8, "uint16_t": C.c_uint16, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}


class AbiError(ValueError):
    def __init__(self, what, where):
        ValueError.__init__(self, "%s in: %s" % (what, " ".join(where.split())))


def _ctype(base, pointers, where):
    if pointers:
        return C.c_char_p if (base, pointers) == ("char", 1) else C.c_void_p
    if base not in _SCALARS:
        raise AbiError("unsupported type '%s'" % base, where)
    return _SCALARS[base]


_DECL = r"([\s*]*)(\w*)\s*((?:\[[^\]]*\]\s*)*)"                      # `*name`, `name[3 * N]`, `name[A][B]`, `name[]`, ``
_FIRST = re.compile(r"\s*(\w+)\b" + _DECL)                            # the type (first word, qualifiers gone) and its declarator
_REST = re.compile(_DECL)
_DIM = re.compile(r"\[([^\]]*)\]")
_PROTO = re.compile(r"\s*([\w\s*]+?)\b(ws_\w+)\s*\(([^()]*)\)\s*")
_CALLED = re.compile(r"\bws_\w+\s*\(")


def _declarators(text, consts, where, array_is_pointer):
    """'float *a, b[2 * N]' -> [(name, ctype)]; a lone type (an unnamed parameter) has the name ''"""
    first, *more = text.split(",")
    found = [_FIRST.fullmatch(first)] + [_REST.fullmatch(d) for d in more]
    if None in found:
        raise AbiError("cannot read '%s'" % " ".join(text.split()), where)
    base = found[0].group(1)
    out = []
    for stars, name, dims in (m.groups()[-3:] for m in found):
        dims = _DIM.findall(dims) if dims else ()
        if array_is_pointer and dims:
            out.append((name, C.c_void_p))
            continue
        t = _ctype(base, stars.count("*"), where)
        for dim in reversed(dims):
            if not re.fullmatch(r"[\w\s+\-*()]+", dim):
                raise AbiError("array extent '%s' is no integer expression" % dim, where)
            try:
                t = t * int(eval(dim, {"__builtins__": {}}, dict(consts)))
            except Exception as e:
                raise AbiError("array extent '%s' (%s)" % (dim, e), where)
        out.append((name, t))
    return out


def parse(text):
    """header text -> Abi(prototypes {name: (restype, [argtypes])}, structs {name: [(field, ctype)]}, constants {name: int})"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S).replace("\\\n", " ")
    consts = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\w+)[ \t]*$", text, flags=re.M)
              if re.fullmatch(r"\d+|0[xX][0-9a-fA-F]+", m.group(2))}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text = re.sub(r'\bextern\s+"C"\s*\{?|\b(?:const|extern)\b', " ", text)

    structs = {}
    for name, body in re.findall(r"\bstruct\s+(ws_\w+)\s*\{([^{}]*)\}", text):
        fields = structs[name] = []
        for stmt in filter(str.strip, body.split(";")):
            where = "struct %s { %s; }" % (name, stmt)
            new = _declarators(stmt, consts, where, array_is_pointer=False)
            if not all(f for f, _ in new):
                raise AbiError("field without a name", where)
            fields += new

    n = 1
    while n:                      # brace blocks (struct / enum / function bodies) end their statement and mark it
        text, n = re.subn(r"\{[^{}]*\}", "@;", text)
    prototypes = {}
    for stmt in re.sub(r"\bstruct\b", " ", text).split(";"):
        if "@" in stmt or not _CALLED.search(stmt):
            continue
        m = _PROTO.fullmatch(stmt)
        if not m:
            raise AbiError("cannot read the declaration", stmt)
        restype = None
        if m.group(1).split() != ["void"]:
            (name, restype), = _declarators(m.group(1), {}, stmt, array_is_pointer=False)
            if name:
                raise AbiError("unsupported return type", stmt)
        args = []
        if m.group(3).strip() not in ("", "void"):
            for p in m.group(3).split(","):
                (_, t), = _declarators(p, consts, stmt, array_is_pointer=True)
                args.append(t)
        prototypes[m.group(2)] = (restype, args)
    return Abi(prototypes, structs, consts)
