"""Texts of one chunk (at most 32 768 bytes) for the LZ77 parse of k_deflate_lz_chunks, shared by
test_deflate_lz_cpu.py (the restatement against zlib) and test_gpu_bgzf_matches.py (the kernel against the restatement).
CASES: {name: text}; what the restatement has to make of each for it to be the case its name says is asserted in test_deflate_lz_cpu.py.
"""
import random

import deflate_lz as Z

M = 32768
STEP = Z.STEP
LETTERS = b"ACGTNacgtn0123456789"
MARKS = bytes(range(0xF0, 0xFA))                                  # bytes no filler holds: a repeat of them is the case's own


def filler(n, seed, letters=LETTERS, clean=True):
    """n bytes of a small alphabet -- compressible by the entropy code alone --; clean: no run of three and no 5-gram twice, so that
    the parse of the filler alone has no match"""
    rng = random.Random(seed)
    out, seen = bytearray(), set()
    while len(out) < n:
        c = letters[rng.randrange(len(letters))]
        if clean:
            if len(out) >= 2 and out[-1] == c and out[-2] == c:
                continue
            if len(out) >= 4:
                g = bytes(out[-4:]) + bytes([c])
                if g in seen:
                    continue
                seen.add(g)
        out.append(c)
    return bytes(out)


def place(text, at, piece):
    text[at:at + len(piece)] = piece


def copy(text, at, dist, length):
    """what an LZ77 match of (length, dist) at `at` stands for, written there"""
    for i in range(length):
        text[at + i] = text[at + i - dist]


def keep_slot(text, src, at, frozen, letters=LETTERS):
    """The table has one entry a hash, the newest: a 4-gram at src is still there when the parse comes to `at` only if no position
    between them has its hash.  Bytes of such positions (never the frozen ones) are changed until none has."""
    h = Z.hash4(text, src)
    for _ in range(64):
        hits = [q for q in range(src + 1, min(at, len(text) - 3)) if Z.hash4(text, q) == h and bytes(text[q:q + 4]) != bytes(text[src:src + 4])]
        if not hits:
            return
        for q in hits:
            j = next(j for j in range(q + 3, q - 1, -1) if j not in frozen)
            text[j] = letters[(letters.index(text[j]) + 7) % len(letters)]
    raise AssertionError("the slot of the 4-gram at %d cannot be kept" % src)


def gram_at_distance(dist, gram=MARKS[:5], n=None):
    """the five bytes `gram` at 0 and again `dist` further on, in clean filler: the repeat is found or not as a whole (its last four
    bytes alone are below DF_LZ_MIN)"""
    n = dist + len(gram) if n is None else n
    text = bytearray(filler(n + len(gram), seed=dist))
    place(text, 0, gram)
    place(text, dist, gram)
    text = text[:n]
    keep_slot(text, 0, dist, set(range(len(gram))) | set(range(dist, dist + len(gram))))
    return bytes(text)


def colliding_grams():
    """two distinct 4-grams of MARKS-like bytes with the restatement's hash equal"""
    seen = {}
    for a in range(0xE0, 0x100):
        for b in range(0xE0, 0x100):
            for c in range(0xE0, 0x100):
                g = bytes([a, b, c, 0xEE])
                h = Z.hash4(g, 0)
                if h in seen:
                    return seen[h], g
                seen[h] = g
    raise AssertionError("no collision")


def collisions():
    """A + tail in step 0, B (another 4-gram, the same hash) in step 1, A + tail again in step 3: the table's newest entry for the
    hash is B's, a false candidate, so the repeat of A is not found; the repeat of a control gram beside it is"""
    a, b = colliding_grams()
    text = bytearray(filler(5 * STEP, seed=77))
    place(text, 10, a + MARKS[:6])
    place(text, 40, MARKS[4:10] + b"##")
    place(text, STEP + 20, b + b"%%")
    place(text, 3 * STEP + 10, a + MARKS[:6])
    place(text, 3 * STEP + 40, MARKS[4:10] + b"##")
    return bytes(text)


def all_distance_codes():
    """a match of twelve bytes for every distance code, at the code's smallest distance and at its largest (the largest a chunk has
    room for): up to 300 at a step's first position, so that the source lies in a step before; the sources of the longer ones are
    filler, never a copy"""
    text = bytearray(filler(M, seed=30))
    at, frozen, copies = 2 * STEP, set(), []
    for c in range(30):
        lo = Z._DIST_BASE[c]
        hi = min(lo + (1 << Z._DIST_EXTRA[c]) - 1, M - STEP)
        for d in (lo, hi):
            at = max(at, d)
            if d <= 300:
                at = (at + STEP - 1) // STEP * STEP
            else:
                while frozen & set(range(at - d - 4, at - d + 16)):
                    at += 13
            assert at + 12 <= M, "no room for distance %d" % d
            copy(text, at, d, 12)
            frozen |= set(range(at, at + 12)) | set(range(at - d, at - d + 12))
            copies.append((at - d, at))
            at += 40
    for src, at in copies:
        keep_slot(text, src, at, frozen)
    return bytes(text)


def period(n, k, seed=5):
    return (filler(k, seed=seed) * (n // k + 1))[:n]


def repeat_to_the_end(cut):
    """a 40-byte piece in step 0 and again at the text's end, the last `cut` bytes of the second one cut off"""
    piece = MARKS + filler(30, seed=9)
    text = bytearray(filler(3 * STEP + 40, seed=10))
    place(text, 20, piece)
    place(text, 3 * STEP, piece)
    return bytes(text[:len(text) - cut])


def deep_distance_code(V=1500, seed=17):
    """Distance frequencies that take an unlimited Huffman code past 15 bits: 17 distance codes with the Fibonacci counts 1, 1, 2, 3 ...
    1597 (4 180 matches) make a tree 16 deep, so df_code_lengths has to halve them.  The table keeps one position a hash, so matches
    thousands of bytes back are found only if nothing between them and their source takes the source's entry.  Hence a vocabulary:
    1 500 words of five bytes whose first 4-grams have a table entry each of their own, laid down once (literals), and then 4 180
    words again, back to back.  A word's match is its last occurrence, at a distance its age decides; every other 4-gram of the text
    (inside a word, across two words, filler) is checked to keep off the words' entries; the byte behind a word differs from the one
    behind its last occurrence, so every match has five bytes.  The nine frequent codes (distances 513 .. 12 288) take turns in
    proportion, each taking the youngest word of its range, so that words age into the longer ranges; the eight rare ones (17 .. 256)
    need a source in the step before and stand at a step's first position, behind up to four bytes of filler."""
    rng = random.Random(seed)
    fib = [1, 1]
    while len(fib) < 17:
        fib.append(fib[-1] + fib[-2])
    rare = dict(zip((8, 9, 10, 11, 12, 13, 14, 15), fib[:8]))
    often = dict(zip((18, 19, 26, 20, 25, 21, 24, 23, 22), fib[8:]))
    letters = bytes(range(0x21, 0x7F))
    words, slots = [], set()
    while len(words) < V:
        w = bytes(rng.choice(letters) for _ in range(5))
        h = Z.hash4(w, 0)
        if h not in slots:
            slots.add(h)
            words.append(w)
    words = [w for w in words if Z.hash4(w, 1) not in slots]      # (the 4-gram inside the word)
    text = bytearray()

    def fits(piece, avoid, word):
        """the piece may follow the text: it does not go on the match before it, and no 4-gram it completes -- but a word's own -- has a word's slot"""
        if piece[0] == avoid:
            return False
        t = text[-3:] + piece
        k = len(t) - len(piece)
        return all(Z.hash4(t, i) not in slots for i in range(len(t) - 3) if not (word and i == k))

    def pad(avoid):
        """a byte of filler that may follow the text and is not the byte in front of it"""
        while True:
            b = rng.choice(letters)
            if fits(bytes([b]), avoid, False) and (not text or b != text[-1]):
                return b

    def span(c):
        return Z._DIST_BASE[c], Z._DIST_BASE[c] + (1 << Z._DIST_EXTRA[c]) - 1

    last, lru = {}, []                                            # a word's last occurrence; the words by it, oldest first
    pool = list(range(len(words)))
    while pool:                                                   # every word once: literals
        i = next((i for i in pool if fits(words[i], None, True)), None)
        if i is None:                                             # none of those left fits behind this byte: another byte
            text.append(pad(None))
            continue
        pool.remove(i)
        last[i] = len(text)
        lru.append(i)
        text += words[i]
    total = dict(often)
    avoid = None
    while any(rare.values()) or any(often.values()):
        at = len(text)
        assert at + 5 <= M, (rare, often)
        to_step = -at % STEP
        if 0 < to_step < 5:                                       # no word across a step's start: filler up to it
            b = pad(avoid)
            text.append(b)
            avoid = None
            continue
        placed = None
        if to_step == 0 and any(rare.values()):
            c = max(c for c in rare if rare[c])
            lo, hi = span(c)
            for i in reversed(lru):                               # the youngest word at a distance of the code
                if at - last[i] > hi:
                    break
                if at - last[i] >= lo and fits(words[i], avoid, True) and text[last[i] - 1] != text[at - 1]:
                    placed = i
                    rare[c] -= 1
                    break
        if placed is None:
            for c in sorted((c for c in often if often[c]), key=lambda c: -often[c] / total[c]):
                lo, hi = span(c)
                for i in reversed(lru):
                    if at - last[i] > hi:
                        break
                    if at - last[i] >= lo and fits(words[i], avoid, True) and text[last[i] - 1] != text[at - 1]:
                        placed = i
                        often[c] -= 1
                        break
                if placed is not None:
                    break
        if placed is None:                                        # no word of a wanted age fits here: a byte of filler
            text.append(pad(avoid))
            avoid = None
            continue
        avoid = text[last[placed] + 5] if last[placed] + 5 < at else None
        lru.remove(placed)
        lru.append(placed)
        last[placed] = at
        text += words[placed]
    b = pad(avoid)
    text.append(b)
    return bytes(text)


def fastq_fixture():
    from test_gpu_bgzf import fastq_text
    return fastq_text()


def build():
    cases = {}
    for d in (255, 256, 257, 32763, 32764):
        cases["gram_at_%d" % d] = gram_at_distance(d, n=M if d > 30000 else d + 300)
    cases["ends_at_n"] = repeat_to_the_end(0)
    cases["cut_by_n"] = repeat_to_the_end(13)
    cases["period_300"] = period(12000 + 77, 300)               # (a match of 258 begins at 300 + 258 k: at 126 mod 128 for k = 41)
    cases["repeat_259"] = filler(300, seed=3)[:259] + b"|" + filler(300, seed=3)[:259] + b"."
    cases["period_2"] = b"ab" * 1500 + b"x"
    cases["period_3"] = b"abc" * 1000 + b"xy"
    cases["one_byte"] = b"A" * 5000
    cases["runs_and_repeats"] = b"aaaaaaab" * 100 + b"ccccccccccd" * 60 + b"aaaaaaab" * 20      # a run of 6 against a repeat 8 back
    cases["collisions"] = collisions()
    cases["no_distance_code"] = filler(3000, seed=12)
    cases["all_distance_codes"] = all_distance_codes()
    cases["deep_distance_code"] = deep_distance_code()
    return cases


CASES = build()
