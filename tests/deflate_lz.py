"""The parse of k_deflate_lz_chunks restated in pure Python, no project code: a chunk in, its token list out.

The parse of a chunk t[0, n) is a function of its bytes alone:
  candidates  in steps of STEP consecutive positions.  Every position p of a step with p + 4 <= n looks up table[h(t[p .. p + 3])],
              which holds the largest position of the steps BEFORE with that hash; then every p of the step enters itself (the
              maximum wins, so the order does not matter).  A source inside the same step is never found.  The candidate is
              compared byte by byte: up to 258 bytes, not past n; another 4-gram with the same hash gives 0.
  runs        a candidate of distance 1: the count of bytes from p on that equal t[p - 1], capped at 258, valid from 3.
  choice      the hash candidate when it has at least MIN bytes and at least 2 more than the (valid) run; else the run when it is
              valid; else a literal.
  selection   greedy from position 0: a token of length L at p makes p + L the next position.
This is the yardstick: the kernel is changed to match it, never the other way round.
"""
STEP = 256
HASH_BITS = 13
MIN = 5
MAX = 258
HASH_MUL = 2654435761


def hash4(t, p):
    """the table slot of the four bytes at p: their little-endian word times HASH_MUL mod 2^32, its top HASH_BITS bits"""
    v = t[p] | t[p + 1] << 8 | t[p + 2] << 16 | t[p + 3] << 24
    return ((v * HASH_MUL) & 0xFFFFFFFF) >> (32 - HASH_BITS)


def common(t, a, b, cap):
    """how many bytes from a and from b on are equal, at most cap"""
    k = 0
    while k < cap and t[a + k] == t[b + k]:
        k += 1
    return k


def candidates(t, min_len=None):
    """per position (length, distance): (1, 0) a literal, else the token the choice rule takes there"""
    min_len = MIN if min_len is None else min_len
    n = len(t)
    table = [-1] * (1 << HASH_BITS)
    out = [(1, 0)] * n
    for s in range(0, n, STEP):
        step = range(s, min(s + STEP, n))
        hashed = [(p, hash4(t, p)) for p in step if p + 4 <= n]
        found = {p: table[h] for p, h in hashed}                  # every look-up of the step comes before its entries
        for p, h in hashed:
            table[h] = max(table[h], p)
        for p in step:
            cap = min(MAX, n - p)
            run = common(t, p - 1, p, cap) if p else 0
            if run < 3:
                run = 0
            q = found.get(p, -1)
            hit = common(t, q, p, cap) if q >= 0 else 0
            if hit >= min_len and hit >= run + 2:
                out[p] = (hit, p - q)
            elif run:
                out[p] = (run, 1)
    return out


def tokens(t, min_len=None):
    """[(position, length, distance)] of the greedy selection; a literal has length 1 and distance 0"""
    cand = candidates(t, min_len)
    out, p = [], 0
    while p < len(t):
        length, dist = cand[p]
        out.append((p, length, dist))
        p += length
    return out


def matches(t, min_len=None):
    """the match tokens alone, in the form deflate_tokens.scan reports them: (text in front, length, distance)"""
    return [tok for tok in tokens(t, min_len) if tok[2]]


def stream_tokens(t, toks):
    """the token list as deflate_tokens.Stream takes it: bytes for literals, (length, distance) for matches"""
    return [bytes(t[p:p + 1]) if not d else (l, d) for p, l, d in toks]


# ---- cost ----------------------------------------------------------------------------------------------------------------------------

_LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
_LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
_DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
              12289, 16385, 24577)
_DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


def symbols(t, toks):
    """(literal/length frequencies with the end-of-block, distance frequencies, extra bits) of a token list"""
    ll, dd, extra = [0] * 286, [0] * 30, 0
    ll[256] = 1
    for p, l, d in toks:
        if not d:
            ll[t[p]] += 1
            continue
        li = max(i for i in range(29) if _LEN_BASE[i] <= l and (i < 28 or l == 258))
        di = max(i for i in range(30) if _DIST_BASE[i] <= d)
        ll[257 + li] += 1
        dd[di] += 1
        extra += _LEN_EXTRA[li] + _DIST_EXTRA[di]
    return ll, dd, extra


def huffman_lengths(freq):
    """unlimited Huffman code lengths of the used symbols (one used symbol: one bit)"""
    import heapq
    heap = [(f, i, (i,)) for i, f in enumerate(freq) if f]
    lens = [0] * len(freq)
    if len(heap) == 1:
        lens[heap[0][1]] = 1
        return lens
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for i in a[2] + b[2]:
            lens[i] += 1
        heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
    return lens


def cost_bytes(t, min_len=None, header=60):
    """what a chunk's block costs by unlimited Huffman codes over the restatement's tokens plus `header` bytes, or its stored form"""
    ll, dd, extra = symbols(t, tokens(t, min_len))
    bits = extra
    for freq in (ll, dd):
        bits += sum(f * l for f, l in zip(freq, huffman_lengths(freq)))
    return min((bits + 7) // 8 + header + 4, len(t) + 5)
