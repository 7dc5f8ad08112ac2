"""The hand-written Python mirror of include/diral_env.h - `SIGNATURES` in diral_amd/_lib.py, the constants and the
`ctypes.Structure` classes of diral_amd/config.py, `ENTRY_DTYPE` of diral_amd/vec_env.py - against the header, the whole
surface and in both directions: every prototype, every field of every struct, every named constant.  The header side comes
from tests/abi_header.py (names by regex, numbers by one gcc probe).  A miscounted signature row raises nothing at run time - a
pointer arrives as an int, a double as a pointer - so this is where it has to show.  No GPU needed."""
import ast
import ctypes
import inspect

from diral_amd import _lib, config
from diral_amd.vec_env import ENTRY_DTYPE
from tests import abi_header as H

# ABI 8, frozen: what a change of the header AND of its mirror in one commit would still have to get past
ABI = 8
SIZES = {"DiralCfg": 88, "DiralNeighborEntry": 16, "DiralSlotPolicy": 168, "DiralRollout": 72, "DiralSlotInfoAge": 40,
         "DiralSlotReplay": 32, "DiralSelect": 168, "DiralMemory": 64, "DiralMemoryAdd": 56, "DiralMemorySample": 120}
OFFSETS = {("DiralSlotReplay", "x_positions"): 8, ("DiralSlotReplay", "T"): 16, ("DiralSlotReplay", "per_env"): 20,
           ("DiralSlotReplay", "xpos_out"): 24, ("DiralRollout", "vel_seed"): 64,
           ("DiralSlotInfoAge", "ia_out"): 8, ("DiralSlotInfoAge", "sum_ia_prev"): 32}
STATUS_CODES = list(range(-11, 0))

INTEGERS = {H.I32: (4, True), H.U32: (4, False), H.I64: (8, True), H.U64: (8, False)}


def mirrors():
    """{struct name: its ctypes class in config.py}."""
    return {n: c for n, c in vars(config).items() if isinstance(c, type) and issubclass(c, ctypes.Structure)}


def is_kind(ctype, kind):
    """Whether a ctypes type is of the header's kind - by class, not by byte width."""
    if kind == H.VOID:
        return ctype is None
    if kind == H.STR:
        return ctype is ctypes.c_char_p
    if kind == H.PTR:
        return ctype is ctypes.c_void_p or (isinstance(ctype, type) and issubclass(ctype, ctypes._Pointer))
    if kind == H.F64:
        return ctype is ctypes.c_double
    if kind == H.F32:
        return ctype is ctypes.c_float
    width, signed = INTEGERS[kind]
    return (isinstance(ctype, type) and issubclass(ctype, ctypes._SimpleCData) and ctype._type_ in "bBhHiIlLqQ"
            and ctypes.sizeof(ctype) == width and (ctype(-1).value < 0) == signed)


# ---- functions ----
def test_header_table_symbols_and_library_name_the_same_functions():
    names = list(H.prototypes())
    assert len(names) >= 52                                      # ABI 8 only adds; and the parser found them
    assert names == list(_lib.SIGNATURES) == _lib.SYMBOLS, "diral_amd/_lib.py and include/diral_env.h disagree"
    lib = _lib.load()
    assert [n for n in names if not hasattr(lib, n)] == []


def test_every_signature_is_of_the_header_s_kinds():
    lib, wrong = _lib.load(), []
    for name, proto in H.prototypes().items():
        restype, argtypes = _lib.SIGNATURES[name]
        fn = getattr(lib, name)
        if fn.restype is not restype or list(fn.argtypes) != list(argtypes):
            wrong.append("%s: bound as something else than its row" % name)
        if not is_kind(restype, proto.ret):
            wrong.append("%s returns %s, the table says %r" % (name, proto.ret, restype))
        if len(argtypes) != len(proto.params):
            wrong.append("%s takes %d arguments, the table has %d" % (name, len(proto.params), len(argtypes)))
        wrong += ["%s argument %d is %s, the table says %r" % (name, i, k, t)
                  for i, (t, k) in enumerate(zip(argtypes, proto.params)) if not is_kind(t, k)]
    assert wrong == []


# ---- structs ----
def test_every_struct_has_its_mirror_field_by_field():
    probe, wrong = H.probe(), []
    assert set(mirrors()) | {"DiralNeighborEntry"} == set(H.structs()) == set(probe.sizes)
    for name, cls in mirrors().items():
        fields = H.structs()[name]
        assert [f for f, _ in cls._fields_] == [f for f, _ in fields], name
        if ctypes.sizeof(cls) != probe.sizes[name]:
            wrong.append("sizeof(%s) is %d, the mirror's %d" % (name, probe.sizes[name], ctypes.sizeof(cls)))
        for (f, ctype), (_, kind) in zip(cls._fields_, fields):
            want, got = probe.fields[name][f], (getattr(cls, f).offset, getattr(cls, f).size)
            if got != want or not is_kind(ctype, kind):
                wrong.append("%s.%s: (offset, size) %r and %s, the mirror has %r and %r" % (name, f, want, kind, got, ctype))
    assert wrong == []


def test_entry_dtype_is_the_neighbour_entry():
    probe, fields = H.probe(), H.structs()["DiralNeighborEntry"]
    assert list(ENTRY_DTYPE.names) == [f for f, _ in fields]
    assert ENTRY_DTYPE.itemsize == probe.sizes["DiralNeighborEntry"]
    for f, kind in fields:
        dt, offset = ENTRY_DTYPE.fields[f][:2]
        assert (offset, dt.itemsize) == probe.fields["DiralNeighborEntry"][f], f
        assert (dt.kind + str(dt.itemsize), dt.byteorder) == ({H.F32: "f4", H.I32: "i4"}[kind], "="), f


# ---- constants ----
def twin(name):
    """The name config.py gives the header's DIRAL_X: X, and DT_X for the enumerators of DiralDType."""
    return ("DT_" if H.constants()[name] == "DiralDType" else "") + name[len("DIRAL_"):]


def config_constants():
    """The upper-case integer constants config.py defines above its first class."""
    names = []
    for node in ast.parse(inspect.getsource(config)).body:
        if isinstance(node, ast.ClassDef):
            break
        if isinstance(node, ast.Assign):
            names += [n.id for t in node.targets for n in ast.walk(t) if isinstance(n, ast.Name)]
    return [n for n in names if n.isupper() and type(getattr(config, n)) is int]


def test_every_constant_has_its_twin_and_its_value():
    values = H.probe().constants
    assert list(values) == list(H.constants()) and len(values) >= 77
    assert sorted(twin(n) for n in values) == sorted(config_constants())
    assert {twin(n): v for n, v in values.items()} == {n: getattr(config, n) for n in config_constants()}


# ---- ABI 8, frozen ----
def test_abi_8_is_what_it_was():
    probe = H.probe()
    assert probe.constants["DIRAL_ABI_VERSION"] == config.ABI_VERSION == _lib.load().diral_env_abi_version() == ABI
    assert probe.sizes == SIZES
    assert dict({n: ctypes.sizeof(c) for n, c in mirrors().items()}, DiralNeighborEntry=ENTRY_DTYPE.itemsize) == SIZES
    assert {k: probe.fields[k[0]][k[1]][0] for k in OFFSETS} == OFFSETS
    assert {(s, f): getattr(mirrors()[s], f).offset for s, f in OFFSETS} == OFFSETS
    assert sorted(v for n, v in probe.constants.items() if n.startswith("DIRAL_ERR_")) == STATUS_CODES
    assert sorted(getattr(config, n) for n in config_constants() if n.startswith("ERR_")) == STATUS_CODES
    assert probe.constants["DIRAL_OK"] == config.OK == 0
