"""The dictionary chain's two record loops inside a context (LEON_CHAIN_FORM=quotient|carry): the worker is fed window by window
while the device resolves, walks and codes the blocks, and finish() hands out its stream.  120 000 reads x 100 bp at k = 31 in blocks
of 50 000 reads: three blocks, and ~20 000 inserted anchors = ~19 segments of the feed.  The stream and the anchor count must be the
same under both forms and equal to the oracle's."""
import pytest

pytestmark = pytest.mark.gpu

K, RPB = 31, 50000


@pytest.fixture(scope="module")
def case():
    import common
    import oracle_lib as O
    bases, off = common.synthetic(120000, 100, 400000, seed=61, err=0.01)
    bl, solid, tai = common.make_bloom(bases, off, K)
    ref = O.encode(bases, off, K, RPB, bl, trace=False)
    assert len(ref.blocks) == 3 and ref.n_anchors > 5 * ((1 << 15) // K)       # several segments
    return bases, off, solid, tai, ref


def _through_context(case, monkeypatch, form):
    import leon_amd
    bases, off, solid, tai, _ = case
    monkeypatch.setenv("LEON_CHAIN_FORM", form)
    ctx = leon_amd.DnaEncodeContext(kmer_size=K, reads_per_block=RPB, bloom_tai=tai, device_id=0)
    try:
        ctx.bloom_insert(solid)
        blocks = ctx.encode_batch(bases, off)
        stream, n_anchors = ctx.finish()
    finally:
        ctx.close()
    return [b[1] for b in blocks], stream, n_anchors


def test_dictionary_stream_is_the_same_under_both_chain_forms(case, monkeypatch):
    ref = case[4]
    got = {form: _through_context(case, monkeypatch, form) for form in ("quotient", "carry")}
    for form, (blocks, stream, n_anchors) in got.items():
        assert n_anchors == ref.n_anchors, form
        assert stream == ref.anchor_dict, form
        assert blocks == ref.blocks, form
    assert got["quotient"][1] == got["carry"][1] and got["quotient"][2] == got["carry"][2]
