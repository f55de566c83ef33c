"""The contract of leon_fastq_split_device / leon_host_fastq_split (include/leon_dna.h) restated in Python -- the text
split at its newlines in one go, the lines grouped in fours -- and the designed texts both forms are tested on.  Not a test file.

CASES: name -> (text, last, max_records, plus_kind).  split(*case) is what a call must give; KNOWN holds, for the cases whose answer
follows from how the text was put together, (n_records, consumed, stop, reason) stated by hand."""
import random

TILE = 4096                 # kernels.h FASTQ_TILE: k_fq_newlines' tile
MAX_GROUPS = 1024           # kernels.h FASTQ_MAX_GROUPS: above that many tiles a workgroup walks more than one
MAX, END, IRREGULAR = 0, 1, 2
R_NONE, R_HEADER, R_PLUS, R_LENGTH, R_PLUS_TEXT, R_PARTIAL = range(6)
ALL = 1 << 62               # a max_records no text reaches


def split(text, last, max_records, plus_kind):
    """-> dict(n_records, consumed, header_bytes, base_bytes, stop, reason, plus_bare, plus_header, headers, header_off, bases, base_off, quals)"""
    text = bytes(text)
    pieces = text.split(b"\n")
    lines, begins, at = [], [], 0
    for p in pieces[:-1]:                                      # the lines that have their newline
        begins.append(at)
        lines.append(p[:-1] if p.endswith(b"\r") else p)
        at += len(p) + 1
    if last and pieces[-1]:                                     # the end of the text ends a line
        begins.append(at)
        lines.append(pieces[-1])
        at = len(text)
    begins.append(at)                                           # where a line behind the last one would begin
    hdr, seq, qual, n, bare, rep, stop, reason = [], [], [], 0, 0, 0, None, R_NONE
    consumed = 0
    while stop is None:
        consumed = begins[min(4 * n, len(lines))]
        if n == max_records:
            stop = MAX
            break
        rec = lines[4 * n:4 * n + 4]
        if len(rec) < 4:
            if last and any(rec):
                stop, reason = IRREGULAR, R_PARTIAL
            else:
                stop = END
                if last:
                    consumed = len(text)
            break
        h, s, p, q = rec
        kind = None
        if not h.startswith(b"@"):
            reason = R_HEADER
        elif not p.startswith(b"+"):
            reason = R_PLUS
        elif len(s) != len(q):
            reason = R_LENGTH
        elif p == b"+":
            kind = 0 if len(h) > 1 else None
        elif p[1:] == h[1:]:
            kind = 1
        else:
            reason = R_PLUS_TEXT
        if reason == R_NONE and kind is not None:
            if plus_kind < 0:
                plus_kind = kind
            if kind != plus_kind:
                reason = R_PLUS_TEXT
        if reason != R_NONE:
            stop = IRREGULAR
            break
        hdr.append(h[1:]); seq.append(s); qual.append(q)
        bare += kind == 0
        rep += kind == 1
        n += 1

    def offsets(parts):
        off = [0]
        for x in parts:
            off.append(off[-1] + len(x))
        return off
    return dict(n_records=n, consumed=consumed, header_bytes=sum(map(len, hdr)), base_bytes=sum(map(len, seq)), stop=stop, reason=reason,
                plus_bare=bare, plus_header=rep, headers=b"".join(hdr), header_off=offsets(hdr), bases=b"".join(seq), base_off=offsets(seq),
                quals=b"".join(qual))


RESULT_FIELDS = ("n_records", "consumed", "header_bytes", "base_bytes", "stop", "reason", "plus_bare", "plus_header")


# ---- the texts ----
def rec(i, L=30, eol=b"\n", plus=b"+", hdr=None, seq=None, qual=None, eols=None):
    """record i: four lines; eols: the four line ends when they differ"""
    h = (b"r%d/%d" % (i, L)) if hdr is None else hdr
    s = bytes(b"ACGTN"[(i + 3 * j) % 5] for j in range(L)) if seq is None else seq
    q = bytes(35 + (i * 7 + j) % 40 for j in range(len(s))) if qual is None else qual
    p = b"+" + h if plus == b"+h" else plus
    e = eols or [eol] * 4
    return b"@" + h + e[0] + s + e[1] + p + e[2] + q + e[3]


def recs(n, first=0, **kw):
    return [rec(first + i, **kw) for i in range(n)]


def exact(total, L=150):
    """records of L bases, the first one's header and the last one's sequence chosen so that the text has exactly `total` bytes"""
    out, size, i = [], 0, 0
    one = len(rec(10 ** 6, L))
    while total - size >= 2 * one + 40:
        out.append(rec(10 ** 6 + i, L)); size += len(out[-1]); i += 1
    left = total - size                                          # one record of `left` bytes: "@" h "\n" s "\n+\n" q "\n" = len(h) + 2 len(s) + 6
    h = b"last" if (left - 6 - 4) % 2 == 0 else b"last."
    out.append(rec(0, (left - 6 - len(h)) // 2, hdr=h))
    text = b"".join(out)
    assert len(text) == total, (len(text), total)
    return text


def newline_at(target, text_recs, eol=b"\n"):
    """the records' text, the first header padded so that a newline lies at byte `target`"""
    text = b"".join(text_recs)
    p = text.rfind(b"\n", 0, target + 1)
    assert p > 0
    text = text_recs[0].replace(eol, b"." * (target - p) + eol, 1) + b"".join(text_recs[1:])
    assert text[target] == 10
    return text


CASES, KNOWN = {}, {}


def case(name, text, last=1, max_records=ALL, plus_kind=-1, known=None):
    assert name not in CASES, name
    CASES[name] = (bytes(text), last, max_records, plus_kind)
    if known is not None:
        KNOWN[name] = known


def _build():
    J = b"".join
    case("empty", b"", 0, known=(0, 0, END, R_NONE))
    case("empty_last", b"", 1, known=(0, 0, END, R_NONE))
    one = rec(0)
    case("one", one, 0, known=(1, len(one), END, R_NONE))
    case("one_last", one, 1, known=(1, len(one), END, R_NONE))
    case("one_open", one[:-1], 0, known=(0, 0, END, R_NONE))
    case("one_open_last", one[:-1], 1, known=(1, len(one) - 1, END, R_NONE))
    for n in (63, 64, 65, 255, 256, 257):                       # the wave and workgroup edges of a lane per record
        t = J(recs(n, L=7))
        case("records_%d" % n, t, n & 1, known=(n, len(t), END, R_NONE))
    for name, size in (("tile", TILE), ("tile_minus_1", TILE - 1), ("tile_plus_1", TILE + 1), ("two_tiles", 2 * TILE)):
        case(name, exact(size), 1, known=None)
    case("newline_ends_tile", newline_at(TILE - 1, recs(40, L=100)))
    case("newline_begins_tile", newline_at(TILE, recs(40, L=100)))
    case("crlf_across_tiles", newline_at(TILE, recs(40, L=100, eol=b"\r\n"), eol=b"\r\n"))
    case("newline_ends_second_tile", newline_at(2 * TILE - 1, recs(80, L=100)))
    big = exact(MAX_GROUPS * TILE + TILE, L=2000)               # a capped grid takes its second turn
    case("past_the_grid_cap", big, 0, known=None)
    case("empty_header", J([rec(0), rec(1, hdr=b""), rec(2)]), known=(3, None, END, R_NONE))
    case("empty_header_only", rec(1, hdr=b"", L=0))
    case("empty_sequences", J([rec(0, L=0), rec(1), rec(2, L=0), rec(3, L=0)]), known=(4, None, END, R_NONE))
    case("sequence_lengths", J(rec(i, L) for i, L in enumerate((1, 15, 16, 17, 64, 63, 65, 128, 129, 2))))
    case("long_sequence", J([rec(0), rec(1, L=TILE + 905), rec(2)]))
    case("quality_begins_with_at", J([rec(0), rec(1, qual=b"@" + b"I" * 29), rec(2, qual=b"@" * 30), rec(3)]), known=(4, None, END, R_NONE))
    case("quality_begins_with_plus", J([rec(0), rec(1, qual=b"+" + b"I" * 29), rec(2)]), known=(3, None, END, R_NONE))
    case("crlf_everywhere", J(recs(70, eol=b"\r\n")), known=(70, None, END, R_NONE))
    case("crlf_on_some_lines", J(rec(i, eols=[(b"\r\n", b"\n")[(i >> j) & 1] for j in range(4)]) for i in range(70)), known=(70, None, END, R_NONE))
    case("lone_cr_inside_lines", J([rec(0), rec(1, seq=b"AC\rGT", qual=b"II\rII"), rec(2, hdr=b"a\rb"), rec(3)]), known=(4, None, END, R_NONE))
    case("cr_cr_lf", J([rec(0), rec(1, L=8, eols=[b"\n", b"\r\r\n", b"\n", b"\r\r\n"]), rec(2)]), known=(3, None, END, R_NONE))
    t = J([rec(0), rec(1, L=8, eols=[b"\n", b"\r\r\n", b"\n", b"\r\n"]), rec(2)])
    case("lengths_differ_by_a_cr", t, known=(1, len(rec(0)), IRREGULAR, R_LENGTH))
    # '+' lines
    for pk in (-1, 0, 1):
        t = J(recs(70))
        case("plus_bare_kind_%d" % pk, t, 1, ALL, pk, known=(70, len(t), END, R_NONE) if pk != 1 else (0, 0, IRREGULAR, R_PLUS_TEXT))
        t = J(recs(70, plus=b"+h"))
        case("plus_header_kind_%d" % pk, t, 1, ALL, pk, known=(70, len(t), END, R_NONE) if pk != 0 else (0, 0, IRREGULAR, R_PLUS_TEXT))
    for j, where in ((0, "first"), (35, "middle"), (69, "last")):
        for a, b, name in ((b"+h", b"+", "bare_among_headers"), (b"+", b"+h", "header_among_bare")):
            rs = [rec(i, plus=b if i == j else a) for i in range(70)]
            # at index 0 the odd one sets the kind: record 1 is then the first to differ
            at = 1 if j == 0 else j
            case("plus_%s_%s" % (name, where), J(rs), known=(at, len(J(rs[:at])), IRREGULAR, R_PLUS_TEXT))
        rs = [rec(i, plus=b"+other" if i == j else b"+") for i in range(70)]
        case("plus_other_text_%s" % where, J(rs), known=(j, len(J(rs[:j])), IRREGULAR, R_PLUS_TEXT))
    case("plus_other_same_length", J([rec(0, plus=b"+h"), rec(1, hdr=b"abc", plus=b"+abd")]), known=(1, len(rec(0, plus=b"+h")), IRREGULAR, R_PLUS_TEXT))
    for pk in (-1, 0, 1):
        rs = [rec(0, plus=b"+h" if pk else b"+"), rec(1, hdr=b""), rec(2, plus=b"+h" if pk else b"+")]
        case("empty_header_bare_plus_kind_%d" % pk, J(rs), 1, ALL, pk, known=(3, None, END, R_NONE))
    # irregular at record j: the prefix is split, consumed points at record j
    R = 70
    for j in (0, 1, 64, R - 1):
        def broken(make, why, name):
            rs = recs(R)
            rs[j] = make(rs[j], j)
            case("%s_at_%d" % (name, j), J(rs), j & 1, known=(j, len(J(rs[:j])), IRREGULAR, why))
        broken(lambda r, i: b"\n" + r, R_HEADER, "blank_line_before")
        broken(lambda r, i: b"\r\n" + r, R_HEADER, "blank_crlf_line_before")
        broken(lambda r, i: b">" + r[1:], R_HEADER, "no_at")
        broken(lambda r, i: rec(i, plus=b"-"), R_PLUS, "no_plus")
        broken(lambda r, i: rec(i, plus=b""), R_PLUS, "empty_third_line")
        broken(lambda r, i: rec(i, qual=b"I" * 29), R_LENGTH, "short_quality")
        broken(lambda r, i: rec(i, seq=b"ACGT\r", qual=b"IIII", eols=[b"\n", b"\r\n", b"\n", b"\n"]), R_LENGTH, "lengths_differ_by_a_cr")
        broken(lambda r, i: rec(i, L=0, qual=b"I"), R_LENGTH, "quality_under_empty_sequence")
    # the end of the text
    body = J(recs(9))
    full = rec(9)
    ends = [i + 1 for i, c in enumerate(full) if c == 10]
    for k in (1, 2, 3):
        for last in (0, 1):
            t = body + full[:ends[k - 1]]
            case("tail_of_%d_lines_last_%d" % (k, last), t, last, known=(9, len(body), IRREGULAR if last else END, R_PARTIAL if last else R_NONE))
            case("tail_of_%d_open_lines_last_%d" % (k, last), t[:-1], last, known=(9, len(body), IRREGULAR if last else END, R_PARTIAL if last else R_NONE))
    case("tail_four_open_lines_no_last", body + full[:-1], 0, known=(9, len(body), END, R_NONE))
    for name, tail in (("one", b"\n"), ("three", b"\n\n\n"), ("crlf", b"\r\n\n\r\n")):
        for last in (0, 1):
            t = body + tail
            case("trailing_blank_%s_last_%d" % (name, last), t, last, known=(9, len(t) if last else len(body), END, R_NONE))
    for last in (0, 1):
        case("trailing_blank_four_last_%d" % last, body + b"\n\n\n\n", last, known=(9, len(body), IRREGULAR, R_HEADER))
    case("blank_lines_only", b"\n\n", 1, known=(0, 2, END, R_NONE))
    case("open_cr_line_last", body + b"\r", 1, known=(9, len(body), IRREGULAR, R_PARTIAL))
    rs = recs(10)
    for m in (0, 1, 9, 10, 11):
        n = min(m, 10)
        case("max_records_%d" % m, J(rs), 1, m, -1, known=(n, len(J(rs[:n])) if m <= 10 else len(J(rs)), MAX if m <= 10 else END, R_NONE))
    case("max_records_before_the_irregular", J(recs(5) + [b"\n"] + recs(5)), 1, 5, -1, known=(5, len(J(recs(5))), MAX, R_NONE))
    # a seeded mix of all of it
    rng = random.Random(20260)
    for draw in range(8):
        n = rng.randrange(150, 400)
        plus = rng.choice([b"+", b"+", b"+h"])
        rs = []
        for i in range(n):
            L = rng.choice([0, 1, 15, 16, 17, 30, 64, 100, 150, 151, rng.randrange(0, 300)])
            q = None
            if L and rng.random() < 0.2:
                q = rng.choice([b"@", b"+"]) + b"J" * (L - 1)
            e = [rng.choice([b"\n", b"\n", b"\n", b"\r\n"]) for _ in range(4)] if draw & 1 else None
            rs.append(rec(i, L, plus=plus, qual=q, eols=e, hdr=b"" if rng.random() < 0.02 and plus == b"+" else None))
        if draw % 4 != 3:                                        # one thing out of order, somewhere
            j = rng.randrange(n)
            rs[j] = rng.choice([lambda r: b"\n" + r, lambda r: b"x" + r, lambda r: r.replace(b"\n+", b"\n-", 1), lambda r: r[:-2] + r[-1:],
                                lambda r: r.replace(b"\n+", b"\n+zz", 1), lambda r: rec(j, 9, plus=b"+h" if plus == b"+" else b"+")])(rs[j])
        t = J(rs)
        if draw % 3 == 0:
            t = t[:len(t) - rng.randrange(0, 200)]
        case("mix_%d" % draw, t, rng.randrange(2), rng.choice([ALL, ALL, n // 2, n]), rng.choice([-1, -1, 0, 1]))


_build()
