"""Reader of include/l4p_hip.h: the C ABI as Python data, and its one mapping to ctypes.

``parse(text)`` reads the header's closed C subset - ``#define L4P_NAME <number>``, ``typedef struct NAME { ... } NAME;`` and
``RET l4p_name(args);`` - and raises ``HeaderError`` naming the declaration for anything else: an ABI addition the reader does not
understand fails at import instead of binding a guessed signature.  ``bind(header)`` turns the reading into ctypes.

The mapping: the scalars of ``SCALARS``; ``char*`` -> ``c_char_p``; a single pointer to a struct of the header -> ``POINTER`` of
its class; ``l4p_stream`` and every other pointer -> ``c_void_p``.  The header does not say which pointers are host pointers, so
host out-parameters (``int* ksize``, ``l4p_engine** out``, ``double* total_ms``) are ``c_void_p`` as well: they take ``byref(...)``,
a ctypes array, ``None`` or an integer address, and ctypes does not check what the pointer points to.
"""
from __future__ import annotations

import ctypes as C
import re
from typing import Dict, List, NamedTuple, Optional, Tuple, Union


class HeaderError(ValueError):
    pass


SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "long long": C.c_longlong, "unsigned long long": C.c_ulonglong,
           "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "char": C.c_char, "unsigned char": C.c_ubyte}


class CType(NamedTuple):
    base: str  # a key of SCALARS, "void", or a typedef name of the header
    const: bool  # of the base type
    ptrs: Tuple[bool, ...]  # one entry per '*', True where a const follows it

    def spell(self) -> str:
        return ("const " if self.const else "") + self.base + "".join("* const" if c else "*" for c in self.ptrs)


class Field(NamedTuple):
    name: str
    type: CType
    dims: Tuple[int, ...]  # int a[4][3] -> (4, 3)


class Proto(NamedTuple):
    ret: CType
    args: Tuple[CType, ...]


class Header(NamedTuple):
    constants: Dict[str, Union[int, float]]
    handles: Tuple[str, ...]  # typedef void* NAME
    opaque: Tuple[str, ...]  # typedef struct NAME NAME
    structs: Dict[str, Tuple[Field, ...]]
    protos: Dict[str, Proto]


def _number(text: str, decl: str) -> Union[int, float]:
    v = text[1:-1].strip() if text.startswith("(") and text.endswith(")") else text
    if re.fullmatch(r"-?\d+", v):
        return int(v)
    if re.fullmatch(r"-?\d+\.\d*f?", v):
        return float(v.rstrip("f"))
    raise HeaderError(f"unreadable constant: {decl!r}")


def _preprocessor(text: str, constants: Dict[str, Union[int, float]]) -> str:
    """Collects the #defines and returns the text without preprocessor lines."""
    out, guard = [], None
    for line in text.split("\n"):
        s = line.strip()
        if not s.startswith("#"):
            out.append(line)
            continue
        s = "#" + s[1:].strip()
        m = re.fullmatch(r"#define\s+(\w+)(?:\s+(\S.*))?", s)
        if m and m.group(2) is not None:
            if m.group(1) in constants:
                raise HeaderError(f"defined twice: {s!r}")
            constants[m.group(1)] = _number(m.group(2), s)
        elif m and m.group(1) == guard:
            pass  # the include guard
        elif re.fullmatch(r"#(ifdef|ifndef|include|endif)\b.*", s) and not s.endswith("\\"):
            g = re.fullmatch(r"#ifndef\s+(\w+)", s)
            guard = g.group(1) if g else guard
        else:
            raise HeaderError(f"unreadable preprocessor line: {s!r}")
    return "\n".join(out)


def _declarations(text: str) -> List[str]:
    """Top-level declarations: split at the ';' outside braces, white space collapsed."""
    text, linkage = re.subn(r'extern\s+"C"\s*\{', "", text)
    out, depth, start = [], 0, 0
    for i, ch in enumerate(text):
        if ch == "{":
            depth += 1
        elif ch == "}":
            depth -= 1
        elif ch == ";" and depth == 0:
            out.append(" ".join(text[start:i].split()))
            start = i + 1
    rest = text[start:].split()
    if rest != ["}"] * linkage:  # what closes the extern "C" blocks, nothing else
        raise HeaderError(f"unreadable end of header: {' '.join(rest)!r}")
    return out


class _Reader:
    def __init__(self) -> None:
        self.header = Header({}, (), (), {}, {})
        self.typedefs: List[str] = []

    def specifiers(self, words: List[str], decl: str) -> Tuple[str, bool, List[str]]:
        """(base type, const, the words left over) of the words in front of a declarator's first '*'."""
        const = "const" in words
        words = [w for w in words if w != "const"]
        for n in (3, 2, 1):
            base = " ".join(words[:n])
            if len(words) >= n and (base in SCALARS or base == "void" or base in self.typedefs):
                return base, const, words[n:]
        raise HeaderError(f"unknown type {' '.join(words)!r} in {decl!r}")

    def declarator(self, base: str, const: bool, tokens: List[str], decl: str) -> Field:
        """'* const * name [4][3]' after its specifiers; the name may be missing (a prototype's unnamed parameter)."""
        ptrs: List[bool] = []
        name, dims, i = "", [], 0
        while i < len(tokens) and tokens[i] in ("*", "const"):
            if tokens[i] == "*":
                ptrs.append(False)
            elif ptrs:
                ptrs[-1] = True
            else:
                const = True
            i += 1
        if i < len(tokens) and tokens[i].isidentifier():
            name, i = tokens[i], i + 1
        while i + 2 < len(tokens) and tokens[i] == "[" and tokens[i + 1].isdigit() and tokens[i + 2] == "]":
            dims.append(int(tokens[i + 1]))
            i += 3
        if i != len(tokens):
            raise HeaderError(f"unreadable declarator {' '.join(tokens)!r} in {decl!r}")
        return Field(name, CType(base, const, tuple(ptrs)), tuple(dims))

    def declare(self, text: str, decl: str) -> List[Field]:
        """'const float* a, b[3]' -> its fields; every token must be a word, '*', '[', ']' or ','."""
        tokens = re.findall(r"\w+|\S", text)
        bad = [t for t in tokens if not (t in ("*", "[", "]", ",") or t.isidentifier() or t.isdigit())]
        if bad or not tokens:
            raise HeaderError(f"unreadable {bad[0] if bad else 'empty declaration'!r} in {decl!r}")
        n = next((i for i, t in enumerate(tokens) if not t.isidentifier()), len(tokens))
        base, const, rest = self.specifiers(tokens[:n], decl)
        if len(rest) > 1:
            raise HeaderError(f"unknown type {' '.join(tokens[:n - 1])!r} in {decl!r}")
        tokens, fields, start = rest + tokens[n:], [], 0
        for i, t in enumerate(tokens + [","]):
            if t == ",":
                fields.append(self.declarator(base, const, tokens[start:i], decl))
                start = i + 1
        return fields

    def struct(self, name: str, body: str, decl: str) -> None:
        if "{" in body or "}" in body:
            raise HeaderError(f"nested struct or union in {decl!r}")
        if not body.rstrip().endswith(";"):
            raise HeaderError(f"unterminated field in {decl!r}")
        fields: List[Field] = []
        for stmt in body.rstrip().rstrip(";").split(";"):
            what = f"'{' '.join(stmt.split())};' of struct {name}"
            for f in self.declare(stmt, what):
                self.value(f.type, what)
                if not f.name or f.name in [g.name for g in fields]:
                    raise HeaderError(f"unnamed or repeated field in {what}")
                fields.append(f)
        self.header.structs[name] = tuple(fields)
        self.typedefs.append(name)

    def value(self, t: CType, decl: str, may_be_void: bool = False) -> None:
        """A type that is held or passed by value must be complete."""
        if not t.ptrs and (t.base in self.header.opaque or (t.base == "void" and not may_be_void)):
            raise HeaderError(f"{t.base} by value in {decl!r}")

    def proto(self, ret: str, name: str, args: str, decl: str) -> None:
        r = self.declare(ret, decl)
        if len(r) != 1 or r[0].name or r[0].dims:
            raise HeaderError(f"unreadable return type in {decl!r}")
        self.value(r[0].type, decl, may_be_void=True)
        params: List[CType] = []
        if args.strip() != "void":
            for a in args.split(","):
                p = self.declare(a, decl)[0]
                if p.dims:
                    raise HeaderError(f"array parameter in {decl!r}")
                self.value(p.type, decl)
                params.append(p.type)
        if name in self.header.protos:
            raise HeaderError(f"declared twice: {decl!r}")
        self.header.protos[name] = Proto(r[0].type, tuple(params))

    def read(self, decl: str) -> None:
        m = re.fullmatch(r"typedef void ?\* ?(\w+)", decl)
        if m:
            self.header = self.header._replace(handles=self.header.handles + (m.group(1),))
            self.typedefs.append(m.group(1))
            return
        m = re.fullmatch(r"typedef struct (\w+) (\w+)", decl)
        if m and m.group(1) == m.group(2):
            self.header = self.header._replace(opaque=self.header.opaque + (m.group(1),))
            self.typedefs.append(m.group(1))
            return
        m = re.fullmatch(r"typedef struct (\w+) ?\{(.*)\} ?(\w+)", decl)
        if m and m.group(1) == m.group(3):
            return self.struct(m.group(1), m.group(2), f"struct {m.group(1)}")
        m = re.fullmatch(r"([^(){}]*?)\b(\w+) ?\(([^{}]*)\)", decl)
        if m and not decl.startswith("typedef"):
            return self.proto(m.group(1), m.group(2), m.group(3), decl)
        raise HeaderError(f"unreadable declaration: {decl[:120]!r}")


def parse(text: str) -> Header:
    text = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    if "/*" in text:
        raise HeaderError("unterminated comment")
    reader = _Reader()
    for decl in _declarations(_preprocessor(text, reader.header.constants)):
        reader.read(decl)
    return reader.header


class Binding(NamedTuple):
    structs: Dict[str, type]  # header name -> ctypes.Structure subclass
    signatures: Dict[str, Tuple[Optional[type], List[type]]]  # function -> (restype, argtypes)


def bind(header: Header) -> Binding:
    structs: Dict[str, type] = {}

    def ctype(t: CType) -> Optional[type]:
        if not t.ptrs:
            if t.base == "void":
                return None
            return C.c_void_p if t.base in header.handles else structs.get(t.base) or SCALARS[t.base]
        if len(t.ptrs) == 1 and t.base == "char":
            return C.c_char_p
        if len(t.ptrs) == 1 and t.base in structs:
            return C.POINTER(structs[t.base])
        return C.c_void_p

    for name, fields in header.structs.items():
        members = []
        for f in fields:
            ft = ctype(f.type)
            for d in reversed(f.dims):
                ft = ft * d
            members.append((f.name, ft))
        structs[name] = type(name, (C.Structure,), {"_fields_": members, "__doc__": f"``{name}`` of include/l4p_hip.h."})
    return Binding(structs, {n: (ctype(p.ret), [ctype(a) for a in p.args]) for n, p in header.protos.items()})
