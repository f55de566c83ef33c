"""The host dictionary chain under both of its record loops (LEON_CHAIN_FORM=quotient|carry, host_rc.h): the same bytes as the
oracle's range coder whatever the form, through capi.host_anchor_dict_encode -- the worker, its helpers and its ring as the
contexts use them.  No GPU.

A segment of the feed is (1 << 15) // k k-mers (1 057 at k = 31, 520 at k = 63) and a segment's last symbol leaves the carry loop
for the plain step, so the anchor counts straddle that boundary; the first 512 symbols of a stream are coded in the plain form
in a short segment of their own.  The skewed streams drive the carry loop's other exits: the saturated range (q > qmm: poly-A),
a range below 2^48 with several bytes leaving at once and the carry-less coder's range reset."""
import functools

import numpy as np
import pytest

SIZES = [2, 5, 5, 2, 3, 3, 3, 2] + [256] * 72
FORMS = ["quotient", "carry"]


@pytest.fixture(scope="module")
def lib():
    import leon_amd
    import os
    if not os.path.exists(leon_amd.lib_path()):
        leon_amd.build_library()
    return leon_amd.load_library()


def _expected(syms):
    import oracle_lib as O
    return O.rc_encode_stream(np.ones(len(syms), dtype=np.uint8), syms, SIZES)   # model 1: alphabet 5


@functools.lru_cache(maxsize=None)
def _uniform(k, n, seed=23):
    """(k-mer words, the oracle's stream) of n uniform k-mers; computed once, shared by both forms, never written to"""
    import oracle_lib as O
    rng = np.random.default_rng(seed + 1000 * k + n)
    ints = [(int(rng.integers(0, 1 << 62)) | (int(rng.integers(0, 1 << 62)) << 62)) & ((1 << (2 * k)) - 1) for _ in range(n)]
    w = O.kwords(k)
    kmers = np.array([[x & 0xFFFFFFFFFFFFFFFF, x >> 64][:w] for x in ints], dtype=np.uint64).reshape(-1)
    syms = np.array([(x >> (2 * (k - 1 - i))) & 3 for x in ints for i in range(k)], dtype=np.uint8)
    kmers.setflags(write=False)
    return kmers, _expected(syms)


@functools.lru_cache(maxsize=None)
def _skewed(kind):
    """the four kinds of test_capi_cpu.test_host_anchor_dict_chain_rare_paths, k = 31"""
    rng = np.random.default_rng(11)
    k = 31
    n = {"polyA": 40000, "skewed": 40000, "two_letter": 40000, "uniform_long": 200000}[kind]
    if kind == "polyA":
        syms = np.zeros(n * k, dtype=np.uint8)
        syms[rng.integers(0, n * k, 50)] = 3
    elif kind == "skewed":
        syms = rng.choice(4, size=n * k, p=[0.97, 0.01, 0.01, 0.01]).astype(np.uint8)
    elif kind == "two_letter":
        syms = (rng.integers(0, 2, n * k) * 2).astype(np.uint8)
    else:
        syms = rng.integers(0, 4, n * k).astype(np.uint8)
    s2 = syms.reshape(n, k).astype(np.uint64)
    kmers = np.zeros(n, dtype=np.uint64)
    for i in range(k):
        kmers = (kmers << np.uint64(2)) | s2[:, i]
    kmers.setflags(write=False)
    return kmers, _expected(syms), n


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k,n", [(31, 1), (31, 2), (31, 1056), (31, 1057), (31, 1058), (31, 30000),
                                 (63, 519), (63, 520), (63, 521), (63, 20000)])
def test_chain_form_matches_oracle_around_segment_ends(lib, monkeypatch, form, k, n):
    from leon_amd import capi
    monkeypatch.setenv("LEON_CHAIN_FORM", form)
    kmers, exp = _uniform(k, n)
    assert capi.host_anchor_dict_encode(kmers, k) == exp


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", ["polyA", "skewed", "two_letter", "uniform_long"])
def test_chain_form_rare_paths(lib, monkeypatch, form, kind):
    from leon_amd import capi
    monkeypatch.setenv("LEON_CHAIN_FORM", form)
    kmers, exp, _ = _skewed(kind)
    assert capi.host_anchor_dict_encode(kmers, 31) == exp


@pytest.mark.parametrize("ring,helpers,spares", [("4", "2", "6"), ("8", "1", "0")])
def test_carry_form_under_other_feed_shapes(lib, monkeypatch, ring, helpers, spares):
    """29 and 39 segments of 24-byte records several times round a small ring, made by two helpers with six spares or by one alone"""
    from leon_amd import capi
    monkeypatch.setenv("LEON_CHAIN_FORM", "carry")
    monkeypatch.setenv("LEON_CHAIN_RING", ring)
    monkeypatch.setenv("LEON_CHAIN_HELPERS", helpers)
    monkeypatch.setenv("LEON_CHAIN_SPARES", spares)
    for k, n in [(31, 30000), (63, 20000)]:
        kmers, exp = _uniform(k, n)
        assert capi.host_anchor_dict_encode(kmers, k) == exp


@pytest.mark.parametrize("form", FORMS)
def test_chain_form_decodes_back(lib, monkeypatch, form):
    """leon_host_anchor_dict_decode gives the k-mers back from either form's stream: a uniform two-word one and the poly-A one"""
    from leon_amd import capi
    monkeypatch.setenv("LEON_CHAIN_FORM", form)
    kmers, exp = _uniform(63, 20000)
    stream = capi.host_anchor_dict_encode(kmers, 63)
    assert stream == exp
    assert np.array_equal(capi.anchor_dict_decode(stream, 20000, 63), kmers)
    kmers, exp, n = _skewed("polyA")
    stream = capi.host_anchor_dict_encode(kmers, 31)
    assert stream == exp
    assert np.array_equal(capi.anchor_dict_decode(stream, n, 31), kmers)
