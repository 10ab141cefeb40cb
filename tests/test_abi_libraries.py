"""What holds for every library of the binding's table (agpl_amd._ffi.LIBRARIES), CPU-only: the header's prototypes, the library's
exports and the table's symbols agree; the types the binding sets follow the header; and the build -- read from make's commands, not
from the Makefile's text -- links each library by default from its own object(s), the extensions against libagpl.so and after it,
removes it in `clean`, and recompiles its object when its public header changes."""
import ctypes as C
import os

import pytest

import abi_support as S
import agpl_amd  # noqa: F401
from agpl_amd import _ffi

LIBS = _ffi.LIBRARIES
EXTENSIONS = LIBS[1:]
by_file = pytest.mark.parametrize("rec", LIBS, ids=[rec.file for rec in LIBS])
# the objects compiled without fused-multiply-add contraction: their results are compared with a host evaluation's, operation by operation
NO_CONTRACTION = {"agpl_sampler.o", "agpl_operators.o", "agpl_synth.o", "agpl_predictive.o", "agpl_sample_y.o", "agpl_likgrad.o",
                  "agpl_quantile.o", "agpl_greedy.o", "agpl_loo.o"}


def make_name(rec):
    return "../" + rec.file


def test_the_table_is_libagpl_and_fifteen_extensions_with_their_public_names():
    assert len(LIBS) == 16 and LIBS[0].file == "libagpl.so" and LIBS[0].key == ""
    assert len({rec.key for rec in LIBS}) == len({rec.file for rec in LIBS}) == len({rec.header for rec in LIBS}) == 16
    for rec in LIBS:
        assert getattr(_ffi, rec.key + "SYMBOLS") == rec.symbols and callable(getattr(_ffi, rec.loader))
        assert getattr(_ffi, rec.key + "LIB_PATH") == os.path.join(os.path.dirname(_ffi.__file__), rec.file)
        assert set(rec.types) <= set(rec.symbols) and len(set(rec.symbols)) == len(rec.symbols)
    everything = [s for rec in LIBS for s in rec.symbols]
    assert len(set(everything)) == len(everything)  # no symbol in two libraries


@by_file
def test_header_exports_and_table_agree(rec):
    protos = S.prototypes(os.path.join(S.INC, rec.header))
    assert sorted(protos) == S.exports(getattr(_ffi, rec.key + "LIB_PATH")) == sorted(rec.symbols)


@by_file
def test_bound_types_follow_the_header(rec):
    protos = S.prototypes(os.path.join(S.INC, rec.header))
    lib = getattr(_ffi, rec.loader)()  # loads, an extension resolving against libagpl.so
    assert getattr(_ffi, rec.loader)() is lib
    for name in rec.symbols:
        ret, args = protos[name]
        restype, argtypes = rec.types.get(name) or (None, None)
        fn = getattr(lib, name)
        if restype is None:
            assert fn.restype is C.c_int  # ctypes' default: nothing was set
        else:
            assert fn.restype is restype is (C.c_char_p if ret == "const char *" else S.ctype(ret)), name
        if argtypes is None:
            assert fn.argtypes is None, name
        else:
            assert list(fn.argtypes) == argtypes == [S.ctype(a) for a in args], name


@by_file
def test_the_default_target_links_it_from_its_own_objects_and_clean_removes_them(rec):
    compiles, links = S.build_commands()
    assert len(compiles) == 26 and len(links) == 16 == len(LIBS)
    objs = S.objects(links[make_name(rec)])
    assert len(objs) == (11 if rec is LIBS[0] else 1)
    assert S.links_exactly(make_name(rec), *objs)
    assert sorted(o for command in links.values() for o in S.objects(command)) == sorted(compiles)  # every object is linked, once


@pytest.mark.parametrize("rec", EXTENSIONS, ids=[rec.file for rec in EXTENSIONS])
def test_an_extension_is_linked_against_libagpl_after_it_as_every_other(rec):
    assert S.linked_like(make_name(rec), *[make_name(other) for other in EXTENSIONS])
    assert S.build_commands(make_name(rec))[1][make_name(rec)] == S.build_commands()[1][make_name(rec)]  # asked for alone: the same command
    core = S.build_commands()[1][S.CORE].split()
    assert "-lagpl" not in core and "-lrocsolver" in core and "-lrocblas" in core


@by_file
def test_a_change_to_its_public_header_recompiles_its_objects(rec):
    objs = S.objects(S.build_commands()[1][make_name(rec)])
    assert set(objs) <= S.recompiled_by("../../include/" + rec.header)


def test_contraction_is_off_for_exactly_the_stated_objects():
    compiles = S.build_commands()[0]
    assert {obj for obj in compiles if S.contraction_off(obj)} == NO_CONTRACTION
    for obj, command in compiles.items():  # and every object is its own source's, compiled with COMMON's flags
        assert " -c %s.hip -o %s" % (obj[:-2], obj) in command and "-fno-slp-vectorize" in command.split(), obj
