"""The contract of leon_fasta_split_device / leon_host_fasta_split (include/leon_dna.h) restated in Python -- the text
split at its newlines in one go, the lines grouped by their header lines -- and the designed texts both forms are tested on.  Not a test
file.

CASES: name -> (text, last, max_records, wrap).  split(*case) is what a call must give; KNOWN holds, for the cases whose answer follows
from how the text was put together, (n_records, consumed, stop, reason) stated by hand (consumed None: not stated)."""
import random

TILE = 4096                 # kernels.h FASTQ_TILE: k_fq_newlines' tile
MAX_GROUPS = 1024           # kernels.h FASTQ_MAX_GROUPS: above that many tiles a workgroup of k_fq_newlines walks more than one
ANY = (1 << 64) - 1         # LEON_FASTA_ANY_WIDTH
MAX, END, IRREGULAR = 0, 1, 2
R_NONE, R_HEADER, R_NO_SEQUENCE, R_EMPTY_LINE, R_WIDTH, R_MULTILINE = range(6)
ALL = 1 << 62               # a max_records no text reaches


def judge(seq, wrap):
    """the reason of the first offending line of a record with the sequence lines seq"""
    if wrap == ANY:
        return R_NONE
    if not seq:
        return R_NO_SEQUENCE                                    # (the header line offends)
    for j, line in enumerate(seq):
        is_last = j == len(seq) - 1
        if not line:
            return R_EMPTY_LINE
        if wrap == 0:
            if not is_last:
                return R_MULTILINE
        elif (len(line) > wrap) if is_last else (len(line) != wrap):
            return R_WIDTH
    return R_NONE


def split(text, last, max_records, wrap):
    """-> dict(n_records, consumed, header_bytes, base_bytes, stop, reason, single_max, next_header, headers, header_off, bases, base_off)"""
    text = bytes(text)
    pieces = text.split(b"\n")
    lines, begins, at = [], [], 0
    for p in pieces[:-1]:                                      # the lines that have their newline
        begins.append(at)
        lines.append(p[:-1] if p.endswith(b"\r") else p)
        at += len(p) + 1
    tail = pieces[-1]                                           # what lies behind the last newline
    if last and tail:                                           # the end of the text ends a line
        begins.append(at)
        lines.append(tail)
    heads = [i for i, l in enumerate(lines) if l.startswith(b">")]
    rec_begin = [begins[i] for i in heads]
    rec_lines = [lines[i + 1:j] for i, j in zip(heads, heads[1:] + [len(lines)])]
    if not last and tail.startswith(b">"):                      # a header line whose first byte is in the text: it ends the record before it
        rec_begin.append(at)
        rec_lines.append([])
    whole = len(rec_begin) if last else max(len(rec_begin) - 1, 0)
    rec_begin.append(len(text))
    hdr, seq, n, stop, reason, single_max, next_header = [], [], 0, None, R_NONE, 0, 0
    no_header = bool(text) and not text.startswith(b">")
    while stop is None:
        consumed = 0 if no_header else rec_begin[n]
        if n == max_records:
            stop = MAX
        elif no_header:
            stop, reason, next_header = IRREGULAR, R_HEADER, rec_begin[0]
        elif n >= whole:
            stop = END
        else:
            reason = judge(rec_lines[n], wrap)
            if reason != R_NONE:
                stop, next_header = IRREGULAR, rec_begin[n + 1]
            else:
                hdr.append(lines[heads[n]][1:])
                seq.append(b"".join(rec_lines[n]))
                if len(rec_lines[n]) == 1:
                    single_max = max(single_max, len(rec_lines[n][0]))
                n += 1

    def offsets(parts):
        off = [0]
        for x in parts:
            off.append(off[-1] + len(x))
        return off
    return dict(n_records=n, consumed=consumed, header_bytes=sum(map(len, hdr)), base_bytes=sum(map(len, seq)), stop=stop, reason=reason,
                single_max=single_max, next_header=next_header, headers=b"".join(hdr), header_off=offsets(hdr), bases=b"".join(seq),
                base_off=offsets(seq))


RESULT_FIELDS = ("n_records", "consumed", "header_bytes", "base_bytes", "stop", "reason", "single_max", "next_header")


# ---- the texts ----
def bases(i, L):
    return bytes(b"ACGTN"[(i + 3 * j) % 5] for j in range(L))


def rec(i, L=30, W=None, eol=b"\n", hdr=None, seq=None, lines=None, eols=None):
    """record i: its header line and L bases on lines of W (None: on one line); lines: the sequence lines as given; eols: per line"""
    h = (b"r%d/%d" % (i, L)) if hdr is None else hdr
    if lines is None:
        s = bases(i, L) if seq is None else seq
        lines = [s] if W is None else [s[a:a + W] for a in range(0, len(s), W)]
    e = eols or [eol] * (len(lines) + 1)
    return b"".join(x + y for x, y in zip([b">" + h] + list(lines), e))


def recs(n, first=0, **kw):
    return [rec(first + i, **kw) for i in range(n)]


CASES, KNOWN = {}, {}


def case(name, text, last=1, max_records=ALL, wrap=ANY, known=None):
    assert name not in CASES, name
    CASES[name] = (bytes(text), last, max_records, wrap)
    if known is not None:
        KNOWN[name] = known


def _build():
    J = b"".join
    for w in (0, 60, ANY):
        tag = "any" if w == ANY else str(w)
        case("empty_w%s" % tag, b"", 0, ALL, w, known=(0, 0, END, R_NONE))
        case("empty_last_w%s" % tag, b"", 1, ALL, w, known=(0, 0, END, R_NONE))
        one = rec(0)
        case("one_w%s" % tag, one, 0, ALL, w, known=(0, 0, END, R_NONE))
        case("one_last_w%s" % tag, one, 1, ALL, w, known=(1, len(one), END, R_NONE))
        case("one_open_w%s" % tag, one[:-1], 0, ALL, w, known=(0, 0, END, R_NONE))
        case("one_open_last_w%s" % tag, one[:-1], 1, ALL, w, known=(1, len(one) - 1, END, R_NONE))
    for n in (63, 64, 65, 255, 256, 257):
        # that many LINES: one record of n - 1 sequence lines (wrapped at 7), and that many RECORDS on one line each
        t = rec(0, 7 * (n - 1) - 3, W=7)
        assert t.count(b"\n") == n
        case("lines_%d" % n, t, 1, ALL, 7, known=(1, len(t), END, R_NONE))
        case("lines_%d_any" % n, t + b">x", 0, ALL, ANY, known=(1, len(t), END, R_NONE))
        t = J(recs(n, L=7))
        case("records_%d" % n, t, n & 1, ALL, 0, known=(n if n & 1 else n - 1, len(t) if n & 1 else None, END, R_NONE))
        case("records_%d_w7" % n, t, 1, ALL, 7, known=(n, len(t), END, R_NONE))
    # records of 1, 2, 3, 64, 65 and 300 lines; last lines of 1, W - 1 and W bytes; a length that is a multiple of W
    W = 60
    t = J(rec(i, W * (k - 1) + tail, W=W) for i, (k, tail) in enumerate(((1, 1), (2, 59), (3, 60), (64, 1), (65, 60), (300, 59), (1, 60), (2, 60), (1, 59))))
    case("record_line_counts", t, 1, ALL, W, known=(9, len(t), END, R_NONE))
    case("record_line_counts_no_last", t, 0, ALL, W, known=(8, None, END, R_NONE))
    case("record_line_counts_any", t, 1, ALL, ANY, known=(9, len(t), END, R_NONE))
    case("record_line_counts_w0", t, 1, ALL, 0, known=(1, None, IRREGULAR, R_MULTILINE))
    for L in (1, 15, 16, 17, 63, 64, 65, 128, 129):             # line lengths
        t = J(rec(i, 3 * L - (i % 2), W=L) for i in range(5))
        case("line_length_%d" % L, t, 1, ALL, L, known=(5, len(t), END, R_NONE))
        t = J(recs(5, L=L))
        case("single_line_length_%d" % L, t, 1, ALL, 0, known=(5, len(t), END, R_NONE))
    t = J([rec(0), rec(1, TILE + 905), rec(2)])
    case("line_longer_than_a_tile", t, 1, ALL, 0, known=(3, len(t), END, R_NONE))
    t = J([rec(0, 100, W=60), rec(1, 5000 * 60, W=60), rec(2, 100, W=60)])
    case("contig_of_5000_lines", t, 1, ALL, 60, known=(3, len(t), END, R_NONE))
    case("contig_of_5000_lines_no_last", t, 0, ALL, 60, known=(2, None, END, R_NONE))
    big = J(recs((MAX_GROUPS + 1) * TILE // len(rec(10 ** 6, 2000)) + 1, first=10 ** 6, L=2000))
    case("past_the_grid_cap", big, 1, ALL, 0, known=(None, len(big), END, R_NONE))
    # line ends
    t = J(recs(70, L=150, W=60, eol=b"\r\n"))
    case("crlf_everywhere", t, 1, ALL, 60, known=(70, len(t), END, R_NONE))
    case("crlf_everywhere_any", t, 0, ALL, ANY, known=(69, None, END, R_NONE))
    t = J(rec(i, 150, W=60, eols=[(b"\r\n", b"\n")[(i >> j) & 1] for j in range(4)]) for i in range(70))
    case("crlf_on_some_lines", t, 1, ALL, 60, known=(70, len(t), END, R_NONE))
    t = J([rec(0), rec(1, seq=b"AC\rGT"), rec(2, hdr=b"a\rb"), rec(3, seq=b"\rACGT")])
    case("lone_cr_inside_lines", t, 1, ALL, 0, known=(4, len(t), END, R_NONE))
    t = J([rec(0, 8), rec(1, 8, eols=[b"\n", b"\r\r\n"]), rec(2, 8)])
    case("cr_cr_lf", t, 1, ALL, 9, known=(3, len(t), END, R_NONE))          # the line is its 8 bases and one '\r'
    case("cr_cr_lf_too_wide", t, 1, ALL, 8, known=(1, len(rec(0, 8)), IRREGULAR, R_WIDTH))
    case("open_cr_line_last", rec(0, 8)[:-1] + b"\r", 1, ALL, 8, known=(0, 0, IRREGULAR, R_WIDTH))     # (the end of the text drops no '\r')
    # what a line may hold
    t = J([rec(0), rec(1, hdr=b""), rec(2)])
    case("empty_header", t, 1, ALL, 0, known=(3, len(t), END, R_NONE))
    t = J([rec(0), rec(1, seq=b"AC>GT"), rec(2, hdr=b"a>b>"), rec(3)])
    case("gt_inside_lines", t, 1, ALL, 0, known=(4, len(t), END, R_NONE))
    t = J([rec(0), rec(1, seq=b";comment"), rec(2)])
    case("line_begins_with_semicolon", t, 1, ALL, 0, known=(3, len(t), END, R_NONE))
    # each reason at records 0, 1, 64 and the last, under the wraps that see it; the same texts under ANY
    R = 70
    for j in (0, 1, 64, R - 1):
        def broken(name, make, whys, single=False, more=0):
            rs = recs(R, L=30) if single else recs(R, L=150, W=60)
            rs[j] = make(j)
            t, before = J(rs), len(J(rs[:j]))
            for w, why in whys.items():
                case("%s_at_%d_w%d" % (name, j, w), t, 1, ALL, w, known=(j, before, IRREGULAR, why))
                if j < R - 1:
                    case("%s_at_%d_w%d_no_last" % (name, j, w), t, 0, ALL, w, known=(j, before, IRREGULAR, why))
            case("%s_at_%d_any" % (name, j), t, 1, ALL, ANY, known=(R + more, len(t), END, R_NONE))
        # (behind a record of 120: behind one of 150 its last line of 30 would offend first, as an inner line of another width)
        broken("blank_line_behind", lambda i: rec(i, 120, W=60) + b"\n", {60: R_EMPTY_LINE})
        broken("blank_line_behind_a_short_line", lambda i: rec(i, 150, W=60) + b"\n", {60: R_WIDTH})
        broken("blank_line_behind_single", lambda i: rec(i) + b"\n", {0: R_MULTILINE}, single=True)
        broken("blank_crlf_line_behind", lambda i: rec(i, 120, W=60, eol=b"\r\n") + b"\r\n", {60: R_EMPTY_LINE})
        broken("blank_line_first", lambda i: rec(i, lines=[b"", bases(i, 30)]), {60: R_EMPTY_LINE, 0: R_EMPTY_LINE}, single=True)
        broken("two_header_lines", lambda i: b">first\n" + rec(i, 150, W=60), {60: R_NO_SEQUENCE}, more=1)
        broken("two_header_lines_single", lambda i: b">first\n" + rec(i), {0: R_NO_SEQUENCE}, single=True, more=1)
        broken("inner_line_short", lambda i: rec(i, lines=[bases(i, 60), bases(i, 59), bases(i, 30)]), {60: R_WIDTH})
        broken("inner_line_long", lambda i: rec(i, lines=[bases(i, 61), bases(i, 60), bases(i, 30)]), {60: R_WIDTH})
        broken("last_line_long", lambda i: rec(i, lines=[bases(i, 60), bases(i, 61)]), {60: R_WIDTH})
        broken("one_line_too_long", lambda i: rec(i, 61), {60: R_WIDTH})
        broken("multiline_among_single", lambda i: rec(i, 90, W=60), {0: R_MULTILINE}, single=True)
        broken("empty_line_then_wide", lambda i: rec(i, lines=[bases(i, 60), b"", bases(i, 99)]), {60: R_EMPTY_LINE})
    t = J(recs(5, L=150, W=60))
    case("header_rule_blank_first", b"\n" + t, 1, ALL, 60, known=(0, 0, IRREGULAR, R_HEADER))
    case("header_rule_text_first", b"ACGT\n" + t, 0, ALL, ANY, known=(0, 0, IRREGULAR, R_HEADER))
    case("header_rule_no_header_at_all", b"ACGT\nACGT", 1, ALL, 0, known=(0, 0, IRREGULAR, R_HEADER))
    case("header_rule_open_header_behind", b"ACGT\n>r", 0, ALL, 0, known=(0, 0, IRREGULAR, R_HEADER))
    case("header_rule_max_0", b"ACGT\n" + t, 1, 0, 60, known=(0, 0, MAX, R_NONE))
    case("blank_lines_only", b"\n\n", 1, ALL, ANY, known=(0, 0, IRREGULAR, R_HEADER))
    # max_records
    rs = recs(10, L=150, W=60)
    for m in (0, 1, 9, 10, 11):
        n = min(m, 10)
        case("max_records_%d" % m, J(rs), 1, m, 60, known=(n, len(J(rs[:n])), MAX if m <= 10 else END, R_NONE))
    t = J(recs(5, L=150, W=60) + [rec(5, 61)] + recs(4, first=6, L=150, W=60))
    case("max_records_before_the_irregular", t, 1, 5, 60, known=(5, len(J(recs(5, L=150, W=60))), MAX, R_NONE))
    case("max_records_past_the_irregular", t, 1, 6, 60, known=(5, len(J(recs(5, L=150, W=60))), IRREGULAR, R_WIDTH))
    # the end of the text: cut inside a header line, inside a sequence line, right behind a newline
    body, full = J(recs(9, L=150, W=60)), rec(9, 150, W=60)
    for name, cut in (("inside_header", 4), ("behind_header", full.index(b"\n") + 1), ("inside_sequence", full.index(b"\n") + 30),
                      ("behind_a_sequence_line", full.index(b"\n") + 62), ("whole", len(full)), ("at_the_gt", 1)):
        t = body + full[:cut]
        case("cut_%s" % name, t, 0, ALL, 60, known=(9, len(body), END, R_NONE))
        case("cut_%s_any" % name, t, 0, ALL, ANY, known=(9, len(body), END, R_NONE))
    case("cut_inside_header_last", body + full[:4], 1, ALL, 60, known=(9, len(body), IRREGULAR, R_NO_SEQUENCE))
    case("cut_inside_header_last_any", body + full[:4], 1, ALL, ANY, known=(10, len(body) + 4, END, R_NONE))
    case("cut_inside_sequence_last", body + full[:full.index(b"\n") + 30], 1, ALL, 60, known=(10, None, END, R_NONE))
    case("cut_nothing_behind", body, 0, ALL, 60, known=(8, len(J(recs(8, L=150, W=60))), END, R_NONE))
    case("trailing_blank_line", body + b"\n", 1, ALL, 60, known=(8, None, IRREGULAR, R_WIDTH))       # (the line of 30 in front of it is an inner line now)
    t = J(recs(9, L=120, W=60)) + b"\n"
    case("trailing_blank_line_behind_a_full_line", t, 1, ALL, 60, known=(8, None, IRREGULAR, R_EMPTY_LINE))
    case("trailing_blank_line_any", body + b"\n", 1, ALL, ANY, known=(9, len(body) + 1, END, R_NONE))
    # a seeded mix of all of it
    rng = random.Random(20261)
    for draw in range(8):
        n = rng.randrange(150, 400)
        W = rng.choice([60, 70, 16, 64])
        rs = []
        for i in range(n):
            L = rng.choice([1, W - 1, W, W + 1, 2 * W, 3 * W + 5, 150, rng.randrange(1, 400)])
            e = None
            if draw & 1:
                e = [rng.choice([b"\n", b"\n", b"\n", b"\r\n"]) for _ in range((L + W - 1) // W + 1)]
            rs.append(rec(i, L, W=W, eols=e, hdr=b"" if rng.random() < 0.02 else None))
        if draw % 4 != 3:                                        # one thing out of order, somewhere
            j = rng.randrange(n)
            rs[j] = rng.choice([lambda r: r + b"\n", lambda r: b">x\n" + r, lambda r: r.replace(b"\n", b"\nA", 2), lambda r: r[:-1] + b"ACGT" * W + b"\n",
                                lambda r: r.replace(b"\n", b"\n\n", 1), lambda r: rec(j, 2 * W + 1, W=W + 1)])(rs[j])
        t = J(rs)
        if draw % 3 == 0:
            t = t[:len(t) - rng.randrange(0, 200)]
        case("mix_%d" % draw, t, rng.randrange(2), rng.choice([ALL, ALL, n // 2, n]), rng.choice([W, W, ANY, 0]))


_build()


# ---- the reader's hand-off rule replayed over the restatement (fastq_reader.cpp: first_fasta_record, split_fasta) ----
class BankNotes:
    """what Bank notes about a FASTA file's line widths (bank.cpp, the FASTA branch of Bank::next), and the mode rule read from it"""

    def __init__(self):
        self.seen, self.wrap, self.ok, self.empty, self.single_max = False, 0, True, False, 0
        self.headers, self.bases, self.reads = [], [], 0

    def take(self, piece):
        """the host parser on a piece of text that ends where its last record ends; returns the records read"""
        lines = piece.split(b"\n")
        if lines[-1] == b"":
            lines.pop()
        lines = [l[:-1] if l.endswith(b"\r") else l for l in lines]
        got, i = 0, 0
        while i < len(lines):
            if not lines[i]:
                i += 1
                continue
            assert lines[i].startswith(b">"), "FASTA data before the first header"
            self.headers.append(lines[i][1:])
            i += 1
            n_lines, last_len = 0, 0
            while i < len(lines) and not lines[i].startswith(b">"):
                if n_lines:
                    if not self.seen:
                        self.seen, self.wrap = True, last_len
                    if last_len != self.wrap or self.wrap == 0:
                        self.ok = False
                last_len = len(lines[i])
                n_lines += 1
                self.bases.append(lines[i])
                i += 1
            if n_lines and last_len == 0:
                self.ok = False
            if self.seen and n_lines and last_len > self.wrap:
                self.ok = False
            if n_lines == 0:
                self.empty = True
            if n_lines == 1:
                self.single_max = max(self.single_max, last_len)
            got += 1
        self.reads += got
        return got

    def width(self):
        return self.wrap if self.seen and self.ok and not self.empty and self.single_max <= self.wrap else 0

    def mode(self):
        if not self.ok or self.empty or (self.seen and self.single_max > self.wrap):
            return ANY
        return self.wrap if self.seen else 0


def replay(text):
    """-> dict(reads, bases, header_bytes, fnv_bases, fnv_headers, fasta_line_width, hand_offs, by_host, by_device)"""
    text = bytes(text)
    notes, hand_offs, by_host, by_device, pos = BankNotes(), 0, 0, 0, 0
    front = 0
    r = split(text, 0, 1, ANY)
    if r["stop"] == IRREGULAR and r["next_header"] < len(text):
        front = r["next_header"]
        r = split(text[front:], 0, 1, ANY)
    first = text[:front + r["consumed"]] if r["n_records"] == 1 else text      # (the file has one record, or none: the end of the file ends it)
    if text:
        by_host += notes.take(first)
        hand_offs += 1
        pos = len(first)
    while pos < len(text):
        r = split(text[pos:], 0, ALL, notes.mode())
        notes.headers.append(r["headers"]); notes.bases.append(r["bases"])
        notes.reads += r["n_records"]
        notes.single_max = max(notes.single_max, r["single_max"])
        by_device += r["n_records"]
        pos += r["consumed"]
        assert r["stop"] in (IRREGULAR, END)
        piece = text[pos:pos + r["next_header"] - r["consumed"]] if r["stop"] == IRREGULAR else text[pos:]
        if piece:
            by_host += notes.take(piece)
            hand_offs += 1
            pos += len(piece)

    def fnv(parts):
        h = 1469598103934665603
        for c in b"".join(parts):
            h = ((h ^ c) * 1099511628211) & ((1 << 64) - 1)
        return h
    return dict(reads=notes.reads, bases=sum(map(len, notes.bases)), header_bytes=sum(map(len, notes.headers)), fnv_bases=fnv(notes.bases),
                fnv_headers=fnv(notes.headers), fasta_line_width=notes.width(), hand_offs=hand_offs, by_host=by_host, by_device=by_device)
