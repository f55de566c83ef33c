"""-m gpu: a destroyed context returns its device memory.

Every member of leon_dna_ctx that owns something releases it in its own destructor (csrc/ctx.h); leon_dna_ctx_destroy has no list of
members to fall behind the struct.  Before that, the walk's path cache (wcache) and the sequential resolution pass's chain_* buffers
were missing from the list: every context that had encoded a batch leaked them at close().

The input is test_gpu_structured.py's first sorted case (it asserts resolve_chain_reads > 0 for it, so the sequential pass's buffers
exist), with LEON_WALK_CACHE_LOG2=22: a walk cache of 2^22 buckets x 64 B = 256 MiB per context.  Three create / encode / finish /
close cycles may grow the device memory in use by less than 128 MiB, half of ONE cache; a library that leaks the cache grows by
3 x 256 MiB.  The card is shared, so the smaller growth of two such rounds counts.

What this does not see: the chain_* buffers are under a megabyte at this size, below the measurement's resolution.  Nothing but the
absence of a list covers them."""
import pytest

import common
import synth

pytestmark = pytest.mark.gpu

MiB = 1 << 20
K, RPB = 31, 1000


def _used():
    import torch
    free, total = torch.cuda.mem_get_info()
    return total - free


def test_a_destroyed_context_returns_its_memory(monkeypatch):
    import leon_amd
    from leon_amd import capi
    monkeypatch.setenv("LEON_WALK_CACHE_LOG2", "22")
    g = synth.make_structured_genome(100000, seed=7)
    b, off = synth.make_structured_reads(g, 20000, 150, seed=8, order="sorted")
    bases = b.tobytes()
    bl, solid, tai = common.make_bloom(bases, off, K)

    def cycle():
        ctx = leon_amd.DnaEncodeContext(kmer_size=K, reads_per_block=RPB, bloom_tai=tai)
        ctx.bloom_upload(bl.bits)
        blocks = ctx.encode_batch(bases, off)
        assert ctx.stats()["resolve_chain_reads"] > 0
        ctx.finish()
        ctx.close()
        capi.device_trim()
        return blocks

    first = cycle()                                            # warm-up: the process's own one-time allocations
    growth = []
    for _ in range(2):
        before = _used()
        for _ in range(3):
            assert cycle() == first, "a later cycle's blocks differ from the first cycle's"
        growth.append(_used() - before)
    print("device memory growth over three cycles, two rounds: %s MiB" % [round(x / MiB, 1) for x in growth])
    assert min(growth) < 128 * MiB, growth
