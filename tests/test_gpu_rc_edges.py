"""-m gpu: the directed streams of tests/rc_edges.py (steps of four bytes and more without a reset, resets on demand, totals of 2^17,
2^20 and just below 2^22, rare steps of two streams on the same and on different step indices; tests/test_rc_edges_cpu.py certifies
them) through the three coders that must agree with the oracle byte for byte: k_rc_encode with rc_coder_tile<false> and <true>, the
host chains behind k_rc_records4 (HostBlockCoder::code / code2), and -- at totals above 2^16 -- the device's decoders (decode_on,
div_u64_u32), on one DNA block of 68 000 reads and one header block of 66 000 headers."""
import functools

import numpy as np
import pytest

import common
import hdr_samples as H
import many_blocks as MB
import oracle_lib as O
import rc_edges as E
import synth

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("rc_chains")]

_ENV = ("LEON_RC_GROUP", "LEON_RC_FAST_TOTAL_LOG2", "LEON_RC_STREAMS_ON_HOST", "LEON_RC_HOST_CHUNKS", "LEON_RC_HOST_THREADS", "LEON_RC_CMP")
_NOT_PACK22 = tuple(n for n in E.NAMES if not n.startswith("pack22"))


def _env(monkeypatch, **env):
    """exactly these switches of the range coder (rc_chains' LEON_RC_HOST_BLOCKS stays as the fixture set it)"""
    for name in _ENV:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def _ctx(k=31, rpb=1000, tai=1000):
    import leon_amd
    return leon_amd.DnaEncodeContext(kmer_size=k, reads_per_block=rpb, bloom_tai=tai)


def _run(ctx, names, short=(), then=(), what=""):
    """the named streams, then the short streams of many_blocks, then the streams named in `then`, in ONE call; every payload against
    the oracle's, the first difference by stream, byte and step"""
    S = E.streams()
    syms, begin = E.pack(names, [s[1] for s in short] + [S[n] for n in then])
    got = ctx.rc_encode_streams(syms, begin)
    want = [E.want()[n] for n in names] + [s[2] for s in short] + [E.want()[n] for n in then]
    labels = list(names) + ["many_blocks stream %d (%s)" % (s[0], MB.KIND_NAMES[MB.kind(s[0])]) for s in short] + list(then)
    assert len(got) == len(want)
    for label, g, w in zip(labels, got, want):
        if g != w:
            at = next((i for i in range(min(len(g), len(w))) if g[i] != w[i]), min(len(g), len(w)))
            step = int(np.searchsorted(np.cumsum(E.profiles()[label].n_bytes), at, side="right")) if label in E.NAMES else -1
            pytest.fail("%s: %s differs from the oracle: %d bytes against %d, the first difference at byte %d (left by step %d)" % (
                what, label, len(g), len(w), at, step))


@functools.lru_cache(maxsize=1)
def _short_streams():
    """six short streams of many_blocks that share pair_a's and pair_b's workgroup at 8 blocks a workgroup: their "leave as it is"
    records run beside the two live chains for some two thousand tiles"""
    out = []
    for kd in (MB.EMPTY, MB.ONE, MB.TILE, MB.TILE1, MB.NARROW, MB.NARROW):
        b = next(b for b in range(MB.N_BLOCKS) if MB.kind(b) == kd and b not in [x[0] for x in out])
        m, v = MB.rc_stream(b)
        out.append((b, (m, v), O.rc_encode_stream(m, v, E.MODEL_SIZES)))
    return tuple(out)


@pytest.mark.parametrize("group", [None, "8"])
def test_device_coder(monkeypatch, group):
    """k_rc_encode, rc_coder_tile<false>: every stream in one call -- one block a workgroup as the launcher picks for so few, and
    eight, where pair_a and pair_b code in lanes 0 and 1 of one coder wave with six short streams in the lanes beside them"""
    _env(monkeypatch, **({} if group is None else dict(LEON_RC_GROUP=group)))
    ctx = _ctx()
    if group is None:
        _run(ctx, E.NAMES, what="one block a workgroup")
    else:
        names = ("pair_a", "pair_b")
        _run(ctx, names, short=_short_streams(), then=tuple(n for n in E.NAMES if n not in names), what="eight blocks a workgroup")
    ctx.close()


@pytest.mark.parametrize("log2_total", ["16", "20"])
def test_exact_division_at_real_totals(monkeypatch, log2_total):
    """rc_coder_tile<true>: the switch to the exact division happens mid-stream, when the pumped model's total passes 2^16 / 2^20,
    and the strikes run through it with quotients above 2^32"""
    _env(monkeypatch, LEON_RC_FAST_TOTAL_LOG2=log2_total)
    ctx = _ctx()
    _run(ctx, _NOT_PACK22, what="exact division from a total of 2^%s on" % log2_total)
    ctx.close()


@pytest.mark.parametrize("chunks", ["1", None, "64"])
def test_host_chains(monkeypatch, chunks):
    """k_rc_records4 -> HostBlockCoder: the seven streams below 2^22 together (code2 pairs them), pack22_host -- the longest stream the
    host chains take, its counts just below 2^22 -- alone, and pack22_device, one symbol longer, with the hook still set: the library
    hands it to the device's coder, and the bytes must be the oracle's all the same (the bytes do not tell which coder ran: its counts
    would still fit the records, so this holds the two sides of the hand-over to the oracle, not the place of the hand-over)"""
    ctx = _ctx()
    for threads in ("1", "2"):
        env = dict(LEON_RC_STREAMS_ON_HOST="1", LEON_RC_HOST_THREADS=threads)
        if chunks is not None:
            env["LEON_RC_HOST_CHUNKS"] = chunks
        _env(monkeypatch, **env)
        what = "host chains, %s chunks, %s threads" % (chunks or "default", threads)
        _run(ctx, _NOT_PACK22, what=what)
        _run(ctx, ("pack22_host",), what=what)
        if threads == "1":
            _run(ctx, ("pack22_device",), what=what + " (beyond the hand-over: the device's coder)")
    ctx.close()


# ---- the decoders at totals above 2^16 -------------------------------------------------------------------------------------------
N_HEADERS = 66000
N_READS = 68000                             # of which more than 2^16 - 256 must anchor (98.7 % do): asserted from the oracle's trace below


@functools.lru_cache(maxsize=1)
def _short_reads():
    """68 000 reads of 36..40 bases with 2 % errors and a few N, from a 20 kb genome"""
    g = synth.make_genome(20000, seed=66)
    b, off = synth.make_reads(g, N_READS, 40, seed=67, err=0.02, n_rate=0.002)
    lens = np.random.default_rng(68).integers(36, 41, size=N_READS)
    keep = (np.arange(40)[None, :] < lens[:, None]).reshape(-1)
    reads_off = np.zeros(N_READS + 1, dtype=np.uint64)
    reads_off[1:] = np.cumsum(lens)
    return b[keep].tobytes(), reads_off


@pytest.mark.parametrize("counts_apart", [None, "0"])
def test_dna_block_with_totals_above_2_16(monkeypatch, counts_apart):
    """one block of 68 000 short reads of which more than 2^16 - 256 anchor: the oracle codes the read size, the anchor position and the
    anchor address once per anchored read, so the byte-count model of each of these numeric groups (256 symbols) ends at a total of
    256 + the anchored reads, above 2^16 (tot = Lw[16] + 240 in the counts_apart layout, and LEON_RC_CMP=0: the other one), as do the
    models of their first bytes.  Encoded == the oracle; then decode_blocks on the device == the input"""
    from leon_amd import capi
    from test_gpu_parity import _full_compare
    _env(monkeypatch, **({} if counts_apart is None else dict(LEON_RC_CMP=counts_apart)))
    k = 15
    bases, off = _short_reads()
    bloom = _bloom(k)
    ref, st = _full_compare(bases, off, k, N_READS, bloom=bloom)
    assert len(ref.blocks) == 1 and ref.block_nreads == [N_READS]
    anchored = int((ref.anchor_pos >= 0).sum())
    print("%d of %d reads anchor: the per-read numeric models end at a total of %d" % (anchored, N_READS, anchored + 256))
    assert anchored + 256 > 1 << 16                                     # the total the byte-count models of the per-read numerics reach
    if counts_apart is None:
        ctx = _ctx(k, N_READS, bloom[2])
        ctx.bloom_upload(bloom[0].bits)
        anchors = capi.anchor_dict_decode(ref.anchor_dict, ref.n_anchors, k)
        got = ctx.decode_blocks(anchors, [(0, ref.blocks[0], N_READS)], [len(bases)])
        ctx.close()
        want = MB.dna_normalised([bases[int(off[i]):int(off[i + 1])] for i in range(N_READS)])
        bad = [i for i in range(min(len(got), N_READS)) if got[i] != want[i]][:5]
        assert len(got) == N_READS and not bad, "reads %r do not round-trip" % bad


@functools.lru_cache(maxsize=1)
def _bloom(k):
    bases, off = _short_reads()
    return common.make_bloom(bases, off, k)


def test_header_block_with_totals_above_2_16(monkeypatch):
    """66 000 headers in one block: the header stream's models pass 2^16; payload == the oracle's, and both device decoders (the
    symbols alone -- leon_header_decode_symbols --, symbols and text) give the headers back"""
    _env(monkeypatch)
    hs = H.sra(N_HEADERS, seed=9)
    ctx = _ctx(31, N_HEADERS, 100000)
    blocks = ctx.header_encode_batch(hs)
    assert [(b[0], b[2]) for b in blocks] == [(0, N_HEADERS)]
    assert blocks[0][1] == O.header_encode_block(hs, hs[0]), "header block differs from the oracle"
    S = ctx.header_symbol_set(blocks)
    got = S.text(0, 1, hs[0])
    S.close()
    assert got == hs, "headers %r differ (symbols on the device)" % [i for i in range(N_HEADERS) if got[i] != hs[i]][:5]
    got, n_host = ctx.header_decode_blocks_device(blocks, hs[0])
    assert got == hs, "headers %r differ (text on the device)" % [i for i in range(N_HEADERS) if got[i] != hs[i]][:5]
    assert n_host == 0, "the block went to the host decoder"
    ctx.close()
