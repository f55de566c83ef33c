"""-m gpu: full default resolution windows against the oracle.  Every other byte comparison with the oracle stops at 50 000 reads, while
the encoder resolves its anchors in windows of 2^21 reads (the first one 2^17): window hand-over, the sequential pass at its natural chunk
(2^19 reads, re-proposal between chunks), the dictionary's growth to hundreds of thousands of keys, anchor addresses coded in three bytes
and the walk's path cache at real occupancy are reached only at that size.  The oracle needs minutes per case there, so
tests/make_golden_window.py ran it once and froze digests of what it computed (tests/golden/self_golden_window.json, SELF-golden);
this file regenerates the same 2.3 M reads (synth.window_reads) and compares the HIP path with them, block by block and stage by stage."""
import hashlib
import json

import pytest

import make_golden_window as W
import synth

pytestmark = pytest.mark.gpu

GOLD = json.load(open(W.PATH))
CASES = {c["id"]: c for c in GOLD["cases"]}
KNOBS = ("LEON_CHAIN_CHUNK", "LEON_RESOLVE_ROUNDS", "LEON_WALK_CACHE", "LEON_WALK_CACHE_LOG2", "LEON_WALK_HOP_LOG2", "LEON_XCH_LOOKUPS")
_inputs, _solid = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release_inputs():
    yield
    _inputs.clear()
    _solid.clear()


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for v in KNOBS:
        monkeypatch.delenv(v, raising=False)


def _sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def _where(case, b):
    blk = case["blocks"][b]
    return "%s: block %d (reads [%d, %d), resolution window %s)" % (case["id"], b, blk["reads"][0], blk["reads"][1],
                                                                     "-".join(str(w) for w in sorted(set(blk["windows"]))))


def _input(cid):
    """the case's reads, generated once per module and checked block by block against the digests the oracle saw"""
    if cid not in _inputs:
        case = CASES[cid]
        bases, off = synth.window_reads(case["spec"])
        assert len(off) - 1 == case["n_reads"] and len(bases) == case["n_bases"], "generator drift in %s: sizes" % cid
        for b, blk in enumerate(case["blocks"]):
            r0, r1 = blk["reads"]
            assert W.input_digests(bases, off[r0:r1 + 1]) == (blk["bases_sha256"], blk["offsets_sha256"]), \
                "generator drift: %s's reads differ from those the golden was made of; regenerate it with python tests/make_golden_window.py " \
                "(and say why in the commit)" % _where(case, b)
        _inputs[cid] = (bases, off)
    return _inputs[cid]


def _device_solid(cid):
    if cid not in _solid:
        from leon_amd import capi
        case = CASES[cid]
        bases, off = _input(cid)
        _solid[cid] = capi.kmer_solid(bases, off, case["k"], case["min_abundance"])
    return _solid[cid]


def _ctx(cid, keep_trace=False):
    """a context with the bloom built on the device from the device's own count"""
    import leon_amd
    case = CASES[cid]
    ctx = leon_amd.DnaEncodeContext(kmer_size=case["k"], reads_per_block=case["reads_per_block"], bloom_tai=case["bloom_tai"],
                                    keep_trace=keep_trace)
    ctx.bloom_insert(_device_solid(cid))
    assert _sha(ctx.bloom_download().tobytes()) == case["bloom_sha256"], "%s: the device's bloom differs from the golden" % cid
    return ctx


def _check_blocks(case, blocks):
    """block ids, read counts and payloads against the golden: the first block that differs, named"""
    nb = len(case["blocks"])
    got = sorted(blocks)
    assert [g[0] for g in got] == list(range(nb)), "%s: block ids %s, want 0 .. %d" % (case["id"], [g[0] for g in got][:8], nb - 1)
    for b, (g, blk) in enumerate(zip(got, case["blocks"])):
        assert g[2] == blk["n_reads"], "%s, stage: block read count" % _where(case, b)
        assert len(g[1]) == blk["size"] and _sha(g[1]) == blk["payload_sha256"], "%s, stage: block payload" % _where(case, b)


def _check_dict(case, d, na):
    assert na == case["n_anchors"], "%s: %d anchors, want %d" % (case["id"], na, case["n_anchors"])
    assert len(d) == case["anchor_dict_bytes"] and _sha(d) == case["anchor_dict_sha256"], "%s: dictionary stream differs" % case["id"]


@pytest.mark.parametrize("cid", list(CASES))
def test_generator_reproduces_the_golden_inputs(cid):
    _input(cid)


@pytest.mark.parametrize("cid", list(CASES))
def test_device_count_and_bloom(cid):
    from leon_amd import capi
    case = CASES[cid]
    k = case["k"]
    solid = _device_solid(cid)
    n_solid = len(solid) // capi.kmer_words(k)
    assert n_solid == case["n_solid"], "%s: %d solid k-mers counted on the device, the oracle %d" % (cid, n_solid, case["n_solid"])
    assert W.solid_digest(solid, k) == case["solid_sha256"], "%s: the device's solid k-mers differ from the oracle's" % cid
    assert max(n_solid * 12, 1000) == case["bloom_tai"]                  # common.make_bloom's size
    _ctx(cid).close()                                                     # bloom_insert == the oracle's bloom, bit for bit


@pytest.mark.usefixtures("rc_chains")
@pytest.mark.parametrize("cid", list(CASES))
def test_one_batch_stage_by_stage(cid):
    case = CASES[cid]
    bases, off = _input(cid)
    n = len(off) - 1
    ctx = _ctx(cid, keep_trace=True)
    blocks = ctx.encode_batch(bases, off)
    pos, addr, flags = ctx.trace_anchors(n)
    ev = ctx.trace_events(int(off[-1]))
    d, na = ctx.finish()
    st = ctx.stats()
    kmers = ctx.anchor_kmers(na)
    ctx.close()
    # stage by stage, as _full_compare: anchors, then events, then bytes, then the dictionary
    spans = [blk["reads"] for blk in case["blocks"]]
    digests = [W.anchor_digests(pos[r0:r1], addr[r0:r1], flags[r0:r1]) for r0, r1 in spans]
    for i, (stage, key) in enumerate((("anchor positions", "anchor_pos_sha256"), ("anchor addresses", "anchor_addr_sha256"),
                                      ("revcomp/inserted flags", "flags_sha256"))):
        for b, blk in enumerate(case["blocks"]):
            assert digests[b][i] == blk[key], "%s, stage: %s" % (_where(case, b), stage)
    for b, (blk, (r0, r1)) in enumerate(zip(case["blocks"], spans)):
        assert _sha(ev[int(off[r0]):int(off[r1])]) == blk["events_sha256"], "%s, stage: walk events" % _where(case, b)
    _check_blocks(case, blocks)
    _check_dict(case, d, na)
    assert _sha(kmers.astype("<u8").tobytes()) == case["anchor_kmers_sha256"], "%s: anchor k-mers differ" % cid
    assert st["n_symbols"] == case["n_symbols"]
    # what the case is there for, from the run itself
    deltas = [W.max_addr_delta(pos[r0:r1], addr[r0:r1]) for r0, r1 in spans]
    assert deltas == [blk["max_addr_delta"] for blk in case["blocks"]]
    assert st["resolve_windows"] == 3 == case["n_windows"]
    print("\n[window] %s: resolve_windows %d, resolve_chain_reads %d (in %d windows), n_anchors %d, largest in-block address delta %d"
          % (cid, st["resolve_windows"], st["resolve_chain_reads"], st["resolve_chain_windows"], na, max(deltas)))
    if cid == "sorted":
        # only the full window can leave more than 2^19 reads to the sequential pass: it ran two natural chunks at least
        assert st["resolve_chain_reads"] > (1 << 19) + (1 << 17) + (case["n_reads"] - (1 << 17) - (1 << 21))
    else:
        assert na > 65536 and max(deltas) >= 65536                       # three-byte address numerics


def test_random_in_two_batches():
    # cut at block 23 (1.15 M reads): neither batch's windows end where the one-batch run's do
    case = CASES["random"]
    bases, off = _input("random")
    cut = 23 * case["reads_per_block"]
    ctx = _ctx("random")
    blocks = ctx.encode_batch(bases, off[:cut + 1])
    assert ctx.stats()["resolve_windows"] == 2
    blocks += ctx.encode_batch(bases, off[cut:])
    d, na = ctx.finish()
    ctx.close()
    _check_blocks(case, blocks)
    _check_dict(case, d, na)


@pytest.mark.parametrize("cid,knobs", [("random", {"LEON_WALK_CACHE": "0"}),
                                       ("random", {"LEON_WALK_CACHE_LOG2": "10", "LEON_WALK_HOP_LOG2": "1"}),
                                       ("pairs63", {"LEON_WALK_CACHE_LOG2": "10"})],
                         ids=["random-no_cache", "random-cache1024_hop1", "pairs63-cache1024"])
def test_walk_cache_off_and_overfull(cid, knobs, monkeypatch):
    # no path cache (what ranks >= 3 run), and a cache of 1024 buckets for millions of walkers: full buckets everywhere
    for key, v in knobs.items():
        monkeypatch.setenv(key, v)
    case = CASES[cid]
    bases, off = _input(cid)
    ctx = _ctx(cid)
    blocks = ctx.encode_batch(bases, off)
    d, na = ctx.finish()
    ctx.close()
    _check_blocks(case, blocks)
    _check_dict(case, d, na)


def test_sorted_as_three_ranks():
    # leon_dna_set_shard(r, 3), the walk divided by anchor and the window look-ups shared out (emulated ranks)
    from leon_amd import capi
    case = CASES["sorted"]
    bases, off = _input("sorted")
    union = []
    for rank in range(3):
        ctx = _ctx("sorted")
        ctx.set_shard(rank, 3)
        ctx.set_exchange(capi.XCH_EMULATE)
        union += ctx.encode_batch(bases, off)
        d, na = ctx.finish()
        ctx.close()
        assert na == case["n_anchors"]
        if rank == 0:
            _check_dict(case, d, na)
        else:
            assert len(d) == 0, "rank %d wrote a dictionary stream" % rank
    _check_blocks(case, union)
