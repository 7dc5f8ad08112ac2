"""The one place in tests/ that reads include/diral_env.h: its prototypes, structs and named constants, and ONE gcc-compiled
probe of it.  The regexes find names and type words only; every number - a size, an offset, the value of `1u << 17` or of an
enumerator without an initialiser - is the compiler's.  Each function computes once per session.  Not a test module:
tests/test_abi_mirror.py compares diral_amd's hand-written mirror with what this returns."""
import collections
import functools
import os
import re
import shutil
import subprocess
import tempfile
import time

import pytest

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "diral_env.h")

# kinds of a parameter, a return value or a struct field: what ctypes has to agree with, class by class
PTR, I32, U32, I64, U64, F32, F64, STR, VOID = "ptr", "i32", "u32", "i64", "u64", "f32", "f64", "str", "void"
_WORDS = {"int": I32, "int32_t": I32, "uint32_t": U32, "int64_t": I64, "uint64_t": U64, "float": F32, "double": F64}

Prototype = collections.namedtuple("Prototype", "name ret params text")      # params: kinds; text: the flattened declaration
Probe = collections.namedtuple("Probe", "sizes fields constants seconds")    # fields: {struct: {field: (offset, size)}}


@functools.lru_cache(maxsize=None)
def code():
    """The header without its comments."""
    with open(HEADER) as fh:
        return re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)


def _kind(decl, named):
    """The kind of `[const] type[*] [name]`."""
    decl = " ".join(decl.split())
    if "*" in decl:
        return STR if decl.replace(" ", "") == "constchar*" else PTR
    words = [w for w in decl.split() if w != "const"]
    if named:
        words.pop()
    assert len(words) == 1 and words[0] in _WORDS, "a type tests/abi_header.py does not know: %r" % decl
    return _WORDS[words[0]]


@functools.lru_cache(maxsize=None)
def prototypes():
    """Every `diral_*` function the header declares, in its order: {name: Prototype}."""
    out = collections.OrderedDict()
    for ret, name, params in re.findall(r"^([A-Za-z_][\w \*]*?)\s*\b(diral_\w+)\s*\(([^()]*)\)\s*;", code(), re.M):
        assert name not in out, name
        params = " ".join(params.split())
        kinds = [] if params == "void" else [_kind(p, named=True) for p in params.split(",")]
        ret = " ".join(ret.split())
        out[name] = Prototype(name, VOID if ret == "void" else _kind(ret, named=False), kinds, "%s %s(%s);" % (ret, name, params))
    return out


@functools.lru_cache(maxsize=None)
def structs():
    """Every `typedef struct X { ... } X;`: {X: [(field, kind), ...]} in declaration order."""
    out = collections.OrderedDict()
    for name, body in re.findall(r"typedef struct (\w+)\s*\{(.*?)\}\s*\1\s*;", code(), re.S):
        fields = []
        for decl in (d.strip() for d in body.split(";")):
            if decl:
                first, *more = decl.split(",")                       # `int32_t T, per_env;`
                kind = _kind(first, named=True)
                assert kind != PTR or not more, decl                 # `T* a, b` would need a kind per declarator
                fields += [(n.split()[-1].strip(" *"), kind) for n in [first] + more]
        assert all(f.isidentifier() for f, _ in fields), (name, fields)
        out[name] = fields
    return out


@functools.lru_cache(maxsize=None)
def constants():
    """Every named constant: {name: the enum's name, or None for an anonymous enum and for a `#define DIRAL_X value`}
    (the include guard has no value and is none)."""
    out = collections.OrderedDict()
    for owner, body in re.findall(r"\benum\s*(\w*)\s*\{(.*?)\}", code(), re.S):
        for item in body.split(","):
            if item.strip():
                out[item.split("=")[0].strip()] = owner or None
    for name in re.findall(r"^#define (DIRAL_\w+)[ \t]+\S", code(), re.M):
        out[name] = None
    assert all(n.isidentifier() and n.startswith("DIRAL_") for n in out), list(out)
    return out


@functools.lru_cache(maxsize=None)
def probe():
    """The header compiled as C: sizeof of every struct, offsetof and size of every field, the value of every constant."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    t0 = time.time()
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HEADER, 'int main(void) {']
    for s, fields in structs().items():
        lines.append('  printf("S %s - %%zu 0\\n", sizeof(%s));' % (s, s))
        for f, _ in fields:
            lines.append('  printf("F %s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (s, f, s, f, s, f))
    for c in constants():
        lines.append('  printf("C %s - %%lld 0\\n", (long long)(%s));' % (c, c))
    lines += ['  return 0;', '}', '']
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "probe.c"), os.path.join(d, "probe")
        with open(src, "w") as fh:
            fh.write("\n".join(lines))
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", src, "-o", exe])
        rows = [r.split() for r in subprocess.check_output([exe], text=True).splitlines()]
    sizes, fields, values = {}, {s: {} for s in structs()}, {}
    for tag, a, b, x, y in rows:
        if tag == "S":
            sizes[a] = int(x)
        elif tag == "F":
            fields[a][b] = (int(x), int(y))
        else:
            values[a] = int(x)
    return Probe(sizes, fields, values, time.time() - t0)
