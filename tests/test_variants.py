"""Which kernel instantiation a launch runs is one value, worked out once per launch (csrc/rt_device.h: rt_trace_variant_of) and mapped
to a kernel by one table per build of rt_kernel.hip (rt_kernel_trace_fast / rt_kernel_trace_strict).  No GPU: the test build's probe rt_test_trace_variant returns the
packed variant of a set of facts and whether the build it belongs to has a kernel for it.

The expectations below are the launch ladders of the revision before the variant value existed, written out by hand:
  rt_retrace<refract, ss2>                     for the list-driven strict launch (never counting),
  strict rt_trace<refract, count, ss2>          for a strict launch (no GRID, no one-wave form),
  product rt_trace<refract, count, ss2, GRID, W1> otherwise, with
      W1   = not count and not refract and not ((scatter and not ss2) or four_waves)      (rt_one_wave_workgroups)
      GRID = not count and not cull_in_lds
  rt_trace_rays<refract>                        for a ray list."""
import ctypes as C
import itertools

import pytest

import rt_host

STRICT, RETRACE, RAYS, REFRACT, COUNT, SS2, GRID, W1 = (1 << i for i in range(8))       # rt_variant_bits
FACTS = ("strict", "retrace", "refract", "count", "ss2", "cull_in_lds", "scatter", "four_waves")   # bit i of the probe's `facts`


@pytest.fixture(scope="module")
def probe(built):
    lib = C.CDLL(rt_host.TEST_LIB_PATH)
    fn = lib.rt_test_trace_variant
    fn.restype, fn.argtypes = C.c_int, [C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_int)]

    def ask(facts):
        bits, has = C.c_uint32(~0 & 0xffffffff), C.c_int(-1)
        assert fn(facts, C.byref(bits), C.byref(has)) == 0
        return bits.value, has.value
    return ask


def expected(strict, retrace, refract, count, ss2, cull_in_lds, scatter, four_waves):
    if retrace:
        return STRICT | RETRACE | (REFRACT if refract else 0) | (SS2 if ss2 else 0)
    common = (REFRACT if refract else 0) | (COUNT if count else 0) | (SS2 if ss2 else 0)
    if strict:
        return STRICT | common
    one_wave = not count and not refract and not ((scatter and not ss2) or four_waves)
    grid = not count and not cull_in_lds
    return common | (GRID if grid else 0) | (W1 if one_wave else 0)


def test_every_combination_of_facts_gives_the_variant_the_old_ladders_chose(probe):
    fast, strict_build = set(), set()
    for f in itertools.product((False, True), repeat=8):
        facts = sum(1 << i for i, on in enumerate(f) if on)
        bits, has = probe(facts)
        assert bits == expected(*f), dict(zip(FACTS, f))
        assert has == 1, dict(zip(FACTS, f))                         # every reachable variant has a kernel
        if bits & (STRICT | RETRACE):
            assert not bits & (GRID | W1)                             # strict and retrace variants: never grid, never one-wave
        if bits & RETRACE:
            assert bits & STRICT and not bits & COUNT                # rt_retrace lives in the strict build and never counts
        if bits & W1:
            assert not bits & (REFRACT | COUNT)
        if bits & COUNT:
            assert not bits & GRID
        assert not bits & RAYS
        (strict_build if bits & STRICT else fast).add(bits)
    rays = set()
    for refract in (False, True):
        for other in (0, 0xfb):                                      # a ray list: refract alone counts
            bits, has = probe(256 | (4 if refract else 0) | other)
            assert bits == STRICT | RAYS | (REFRACT if refract else 0) and has == 1
            rays.add(bits)
    # the instantiations the two builds emit, no more and no fewer
    assert len(fast) == 16                                           # REFRACT x SS2 x GRID four-wave 8, SS2 x GRID one-wave 4, REFRACT x SS2 counting 4
    assert len([b for b in fast if b & W1]) == 4 and len([b for b in fast if b & COUNT]) == 4
    assert len([b for b in strict_build if not b & RETRACE]) == 8    # rt_trace: REFRACT x COUNT x SS2
    assert len([b for b in strict_build if b & RETRACE]) == 4        # rt_retrace: REFRACT x SS2
    assert len(rays) == 2                                            # rt_trace_rays: REFRACT
    assert len(strict_build | rays) == 14


def test_the_probe_wants_its_outputs(probe, built):
    lib = C.CDLL(rt_host.TEST_LIB_PATH)
    lib.rt_test_trace_variant.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p]
    assert lib.rt_test_trace_variant(0, None, None) != 0
