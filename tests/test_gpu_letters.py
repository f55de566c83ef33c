"""-m gpu: leon_letters_count_device, leon_letters_take_device and leon_letters_apply_device (letters_kernels.hip) against the numpy
model of letters_shapes.py -- never against the code under test.  The bases lie in device memory between two canaries, at base + 5 (an
odd address); the canaries, and what lies behind the host tables, come back unchanged."""
import ctypes as C

import numpy as np
import pytest

import letters_shapes as S

pytestmark = pytest.mark.gpu

CANARY = 64
SHIFT = 5
FILL = 0xA5
SLACK = 8                  # elements behind each host table that a call must leave alone
TABLE_FILL = 0x5A


class OnDevice:
    """`data` (uint8 array) uploaded between two canaries, d_bases = base + CANARY + shift"""

    def __init__(self, data, shift=SHIFT):
        from leon_amd import capi
        self.capi, self.lib, self.n, self.shift = capi, capi.load_library(), len(data), shift
        self.edge = np.full(CANARY + shift, FILL, dtype=np.uint8)
        self.base = capi.device_alloc(CANARY + shift + self.n + CANARY)
        assert self.base % 16 == 0
        self.ptr = self.base + CANARY + shift
        self.lead = self.ptr % 16
        for at, a in ((0, self.edge), (CANARY + shift, data), (CANARY + shift + self.n, self.edge[:CANARY])):
            self.upload(self.base + at, a)

    def upload(self, dst, a):
        if len(a):
            a = np.ascontiguousarray(a)
            assert self.lib.leon_device_upload(0, C.c_void_p(dst), C.c_void_p(a.ctypes.data), len(a)) == 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.capi.device_free(self.base)

    def bytes(self, at=0, n=None):
        n = self.n - at if n is None else n
        return np.frombuffer(self.capi.device_download(self.ptr + at, n), dtype=np.uint8) if n else np.zeros(0, dtype=np.uint8)

    def canaries(self):
        assert self.capi.device_download(self.base, CANARY + self.shift) == self.edge.tobytes(), "bytes in front of d_bases were written"
        assert self.capi.device_download(self.ptr + self.n, CANARY) == self.edge[:CANARY].tobytes(), "bytes behind d_bases were written"

    def count(self):
        return self.capi.letters_count_device(self.ptr, self.n)

    def take(self, n_runs, n_odd):
        """the tables, after the check that the call left their slack alone"""
        runs, pos, byte = self.capi.letters_take_device(self.ptr, self.n, n_runs, n_odd, slack=SLACK, fill=TABLE_FILL)
        assert np.all(runs[2 * n_runs:] == TABLE_FILL) and np.all(pos[n_odd:] == TABLE_FILL) and np.all(byte[n_odd:] == TABLE_FILL), "a table was written past its end"
        return runs[:2 * n_runs].reshape(-1, 2), pos[:n_odd], byte[:n_odd]

    def apply(self, runs, pos, byte):
        self.capi.letters_apply_device(self.ptr, self.n, runs, pos, byte)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        at = np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1))[:4]
        raise AssertionError("%s: differs at %s: got %s, want %s" % (what, at.tolist(), got[at].tolist(), want[at].tolist()))


def check(data, shift=SHIFT, name=""):
    """count, take, the folded buffer, apply on the device and on the host threads: all against the model"""
    from leon_amd import capi
    m = S.Model(data)
    with OnDevice(data, shift) as d:
        assert d.count() == (m.n_runs, m.n_odd), name
        same(d.bytes(), data, name + ": count wrote to the buffer")
        runs, pos, byte = d.take(m.n_runs, m.n_odd)
        same(runs, m.runs, name + ": runs")
        same(pos, m.odd_pos, name + ": odd_pos")
        same(byte, m.odd_byte, name + ": odd_byte")
        folded = d.bytes()
        same(folded, m.folded, name + ": the folded buffer")
        d.canaries()
        d.apply(runs, pos, byte)
        same(d.bytes(), data, name + ": apply on the device")
        d.canaries()
        on_host = folded.copy()
        capi.host_letters_apply(on_host, runs, pos, byte)
        same(on_host, data, name + ": apply on the host threads")


def test_a_line_read_by_eye():
    with OnDevice(np.frombuffer(b"ACgtnNRr.acGT-y", dtype=np.uint8)) as d:
        assert d.count() == (4, 5)
        runs, pos, byte = d.take(4, 5)
        assert runs.tolist() == [[2, 5], [7, 8], [9, 11], [14, 15]] and pos.tolist() == [6, 7, 8, 13, 14] and byte.tobytes() == b"Rr.-y"
        assert d.bytes().tobytes() == b"ACGTNNNNNACGTNN"
        d.apply(runs, pos, byte)
        assert d.bytes().tobytes() == b"ACgtnNRr.acGT-y"
        d.canaries()


@pytest.mark.parametrize("n", S.EDGE_LENGTHS)
def test_every_pointer_alignment(n):
    for shift in range(16):
        check(S.mixed(n, 40 + n, 0.1, 0.1), shift=shift, name="n %d shift %d" % (n, shift))
        if n:
            check(S.lower(S.plain(n, 41), 0, n), shift=shift, name="n %d shift %d, lower-case" % (n, shift))


def test_small_shapes():
    for name, data in S.small_shapes(lead=SHIFT):
        check(data, name=name)


@pytest.mark.parametrize("shift", [0, 5, 15])
def test_runs_at_tile_wave_and_workgroup_joins(shift):
    """the in-place hazard: a workgroup's first bit is the one recorded before anything was folded"""
    check(S.boundaries(shift), shift=shift, name="boundaries")
    check(S.lower(S.plain(6 * S.TILE, 42), 0, 6 * S.TILE), shift=shift, name="six tiles lower-case")


def test_past_the_grid_cap():
    """every workgroup walks a second and a third tile, the ranks carried from tile to tile"""
    data, per = S.past_the_grid_cap(SHIFT)
    assert per >= 3 and len(data) // S.TILE >= 3 * S.MAX_GROUPS
    check(data, name="past the grid cap")


def test_random_draws():
    for i, data in enumerate(S.random_draws(200)):
        check(data, shift=i % 16, name="draw %d" % i)


def test_past_4_gib():
    data, runs, pos, byte, places = S.huge()
    with OnDevice(data) as d:
        del data
        assert d.count() == (len(runs), len(pos))
        got = d.take(len(runs), len(pos))
        same(got[0], runs, "runs"); same(got[1], pos, "odd_pos"); same(got[2], byte, "odd_byte")
        for p, _, folded in places:
            assert d.bytes(p, 1)[0] == folded, p
        assert d.count() == (0, 0)
        d.canaries()
        d.apply(runs, pos, byte)
        for p, original, _ in places:
            assert d.bytes(p, 1)[0] == original, p
        assert d.count() == (len(runs), len(pos))
        d.canaries()
        # every other byte is the 'A' it was
        changed = np.array([p for p, _, _ in places])
        for a in range(0, d.n, 1 << 28):
            part = d.bytes(a, min(1 << 28, d.n - a)).copy()
            part[changed[(changed >= a) & (changed < a + len(part))] - a] = ord("A")
            assert np.all(part == ord("A")), "a byte outside the tables changed near %d" % a


@pytest.mark.parametrize("d_runs,d_odd", [(1, 0), (-1, 0), (0, 1), (0, -1)])
def test_take_with_wrong_counts_changes_nothing(d_runs, d_odd):
    from leon_amd import capi
    data = S.edges()
    m = S.Model(data)
    with OnDevice(data) as d:
        with pytest.raises(capi.LeonDnaError) as e:
            capi.letters_take_device(d.ptr, d.n, m.n_runs + d_runs, m.n_odd + d_odd, slack=SLACK, fill=TABLE_FILL)
        assert e.value.code == -4 and "holds %d run(s) and %d other byte(s)" % (m.n_runs, m.n_odd) in str(e.value)
        for table in e.value.tables:
            assert np.all(table == TABLE_FILL), "a refused call wrote to a table"
        same(d.bytes(), data, "a refused call wrote to the buffer")
        d.canaries()


def test_apply_with_empty_tables_changes_nothing():
    data = S.edges()
    with OnDevice(data) as d:
        d.apply(None, None, None)
        d.apply(np.zeros((0, 2), dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint8))
        same(d.bytes(), data, "apply with empty tables")
        d.canaries()
    # a buffer without such letters: nothing to take, and take leaves it alone
    data = S.plain(3 * S.TILE + 7, 43)
    with OnDevice(data) as d:
        assert d.count() == (0, 0)
        assert [len(a) for a in d.take(0, 0)] == [0, 0, 0]
        same(d.bytes(), data, "take on plain bases")
        d.canaries()
