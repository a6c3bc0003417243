"""The C-ABI library loads without a GPU and exports every symbol include/simplyp.h declares; the ctypes
mirrors match the header's struct layout."""

import ctypes as C
import functools
import inspect
import os
import re

import pytest

from simplyp_amd import abi, engine, marshal

from c_header import c_values, header_text


def test_library_exports_every_declared_symbol():
    engine.build()
    L = engine.lib()
    declared = set(re.findall(r'\b(simplyp_[a-z0-9_]+)\s*\(', header_text()))
    assert declared == set(engine.ABI_SYMBOLS), declared ^ set(engine.ABI_SYMBOLS)
    for name in declared:
        assert hasattr(L, name), name
    # the one place the number is written out: a bump is a deliberate edit here
    assert L.simplyp_abi_version() == abi.ABI_VERSION == int(re.search(r'#define SIMPLYP_ABI_VERSION (\d+)', header_text()).group(1)) == 18


def test_enums_match_python_tables():
    txt = header_text()
    pm = re.search(r'enum \{\s*SIMPLYP_PM_F_QUICK = 0(.*?)SIMPLYP_NP_M', txt, re.S).group(0)
    assert len(re.findall(r'SIMPLYP_PM_[A-Z0-9_]+', pm)) == marshal.NP_M
    pr = re.search(r'enum \{\s*SIMPLYP_PR_A_CATCH = 0(.*?)SIMPLYP_NP_R', txt, re.S).group(0)
    assert len(re.findall(r'SIMPLYP_PR_[A-Z0-9_]+', pr)) == marshal.NP_R
    out = re.search(r'enum \{\s*SIMPLYP_OUT_VSA = 0(.*?)SIMPLYP_N_OUT', txt, re.S).group(0)
    assert len(re.findall(r'SIMPLYP_OUT_[A-Z0-9_]+', out)) == marshal.N_OUT == 25
    assert marshal.MASK_REACH5 == (1 << 3) | (1 << 5) | (1 << 7) | (1 << 9) | (1 << 11)
    # the 26th column (per-member snow depth) sits right after the reference's 25, in the header, the Python tables and the oracle
    tail = re.search(r'SIMPLYP_N_OUT_REF,(.*?)SIMPLYP_N_OUT\b', txt, re.S).group(1)
    assert re.findall(r'SIMPLYP_OUT_[A-Z0-9_]+', re.sub(r'/\*.*?\*/', '', tail, flags=re.S)) == ['SIMPLYP_OUT_D_SNOW']
    assert re.search(r'SIMPLYP_OUT_D_SNOW\s*=\s*SIMPLYP_N_OUT_REF\s*,\s*SIMPLYP_N_OUT\b', re.sub(r'/\*.*?\*/', '', txt, flags=re.S))
    assert marshal.ALL_COLUMNS.index('D_snow') == marshal.N_OUT == 25 and len(marshal.ALL_COLUMNS) == 26
    assert marshal.MASK_D_SNOW == 1 << 25 and marshal.MASK_ALL == (1 << 25) - 1
    gv = re.search(r'SIMPLYP_GOF_Q = 0(.*?)SIMPLYP_N_GOF_VARS', txt, re.S).group(0)
    assert [n.lower() for n in re.findall(r'SIMPLYP_GOF_([A-Z]+)', gv)] == [v.lower() for v in abi.GOF_VARS]
    gs = re.search(r'SIMPLYP_GOFSTAT_N_OBS = 0(.*?)SIMPLYP_N_GOF_STATS', txt, re.S).group(0)
    assert len(re.findall(r'SIMPLYP_GOFSTAT_[A-Z0-9_]+', gs)) == len(abi.GOF_STATS) == 8


STRUCTS = [cls for _, cls in inspect.getmembers(abi, inspect.isclass) if issubclass(cls, C.Structure) and hasattr(cls, '_fields_')]


@functools.lru_cache(maxsize=None)
def layout_values():
    """sizeof of every mirrored struct, offsetof and sizeof of every field: one run of the C compiler for all the cases."""
    exprs = []
    for cls in STRUCTS:
        if 'c_name' in vars(cls):
            exprs.append('sizeof(%s)' % cls.c_name)
            for f, _ in cls._fields_:
                exprs += ['offsetof(%s, %s)' % (cls.c_name, f), 'sizeof(((%s*)0)->%s)' % (cls.c_name, f)]
    return c_values(exprs)


@pytest.mark.parametrize('cls', STRUCTS, ids=lambda cls: cls.__name__)
def test_struct_layouts(cls):
    """A ctypes mirror vs its struct in include/simplyp.h: the header's field names, and the C compiler's offset and size of every
    field and size of the struct."""
    assert 'c_name' in vars(cls), 'abi.%s does not name its struct of the header' % cls.__name__
    body = re.search(r'typedef struct \{([^{}]*)\}\s*%s\s*;' % cls.c_name, re.sub(r'/\*.*?\*/', ' ', header_text(), flags=re.S))
    assert body, 'the header has no struct %s' % cls.c_name
    assert abi.structs()[cls.c_name] is cls
    # every field and no other: tail padding can keep the size of a struct that lost its last field
    assert [f for f, _ in cls._fields_] == re.findall(r'(\w+)\s*(?:\[\w+\])?\s*[,;]', body.group(1)), cls.c_name
    got = layout_values()
    for f, _ in cls._fields_:
        where = '%s.%s' % (cls.c_name, f)
        assert got['offsetof(%s, %s)' % (cls.c_name, f)] == getattr(cls, f).offset, where
        assert got['sizeof(((%s*)0)->%s)' % (cls.c_name, f)] == getattr(cls, f).size, where
    assert got['sizeof(%s)' % cls.c_name] == C.sizeof(cls), cls.c_name


def test_every_struct_of_a_prototype_has_a_mirror():
    """A struct pointer without a class in abi.py would be bound as a plain c_void_p, unchecked."""
    txt = re.sub(r'/\*.*?\*/', ' ', header_text(), flags=re.S)
    declared = set(re.findall(r'\}\s*(simplyp_\w+)\s*;', re.sub(r'typedef enum \{.*?\}', '', txt, flags=re.S)))
    named = set(re.findall(r'\b(simplyp_\w+)\s*\*', txt)) & declared
    assert named and named <= set(abi.structs()), named - set(abi.structs())
    assert len(STRUCTS) == len(abi.structs()) and set(abi.structs()) <= declared


def test_prototypes_are_the_headers():
    """The argtypes and restypes the binding derives from the header, pinned where the widths and kinds mix."""
    vp, i32, info = C.c_void_p, C.c_int32, C.POINTER
    proto = {name: (restype, argtypes) for name, restype, argtypes in engine.prototypes(header_text())}
    assert list(proto) == engine.ABI_SYMBOLS and len(proto) == 51
    assert set(proto) == set(re.findall(r'\b(simplyp_[a-z0-9_]+)\s*\(', header_text()))
    assert proto['simplyp_quantiles'][1] == [vp, i32, C.c_int64, vp, vp, vp, vp, i32, vp, info(abi.QuantileInfo)]
    assert proto['simplyp_pf_jitter'][1] == [vp, i32, i32, C.c_uint64, C.c_uint32, C.c_double] + [vp] * 8 + [info(abi.PfInfo)]
    assert proto['simplyp_ctx_create'][1] == [C.c_int, vp]
    assert proto['simplyp_last_error'][0] is C.c_char_p and proto['simplyp_host_alloc'][0] is vp
    assert proto['simplyp_out_bytes'][0] is C.c_int64 and proto['simplyp_ctx_destroy'][0] is None
    engine.build()
    L = engine.lib()                                               # ... and they are what the loaded library carries
    for name, (restype, argtypes) in proto.items():
        assert getattr(L, name).restype is restype and list(getattr(L, name).argtypes) == argtypes, name


@pytest.mark.parametrize('name,decl', [('simplyp_x', 'int simplyp_x(float v);'), ('simplyp_y', 'int simplyp_y(int (*cb)(int));')])
def test_parser_refuses_what_it_cannot_type(name, decl):
    with pytest.raises(engine.EngineError, match=name):
        engine.prototypes('int simplyp_ok(int32_t a);\n' + decl)


def test_out_bytes_and_host_argument_errors():
    L = engine.lib()
    dims = abi.Dims(100, 3, 366, 1)
    opts = abi.make_opts(out_mask=marshal.MASK_REACH5)
    assert L.simplyp_out_bytes(C.byref(dims), C.byref(opts), 0) == 5 * 366 * 3 * 100 * 8
    assert L.simplyp_out_bytes(C.byref(dims), C.byref(opts), 1) == 5 * 366 * 1 * 100 * 8
    # no device here: creating a context fails with a message, never a crash
    h = C.c_void_p()
    if L.simplyp_device_count() == 0:
        assert L.simplyp_ctx_create(0, C.byref(h)) < 0
        assert b'not available' in L.simplyp_last_error(None)


def test_no_kernel_uses_scratch():
    """Every kernel of the library keeps its state in registers: hipcc's resource remarks (no GPU needed) show 0 bytes of scratch
    per lane for all of them.  The snow instantiation of the chain kernel spilled 20 B per lane until round 4."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(engine.HERE), 'tools'))
    import resource_usage
    asm = {}
    rows = resource_usage.resource_usage(asm_of=asm)
    big = [r for r in rows if 'chain_kernel' in r['name'] or 'queue_kernel' in r['name']]
    assert len(big) == 26 and len(rows) >= 36, [r['name'] for r in rows]
    assert all(r['Occupancy [waves/SIMD]'] >= 1 for r in rows)
    spilled = {r['name']: r['ScratchSize [bytes/lane]'] for r in rows if r['ScratchSize [bytes/lane]'] != 0}
    assert not spilled, spilled
    # The kernels that switch pairs lane by lane read their tableau row from LDS; every read is issued well ahead of the s_waitcnt that
    # needs it (one stage's right-hand side, ~60 instructions).  Left to the compiler the reads sat 5-8 instructions before their waits
    # -- eight exposed LDS round trips per attempt (profiles/r04_experiments.md, section 6).
    for kern in ('simplyp_queue_kernelILi2ELb0ELi1ELb1', 'simplyp_queue_kernelILi2ELb0ELi4ELb1', 'simplyp_chain_kernelILi2ELb1ELi1ELb1'):
        c = resource_usage.lds_read_cover(asm['asm'], kern)
        assert c['ds_reads'] >= 10 and c['block_instructions'] > 300, (kern, c)
        assert min(c['cover']) >= 20, (kern, c)          # (5-8 before; the four-lane kernel's stages are a third as long)
