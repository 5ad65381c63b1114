"""Structured inputs for the fill kernels' walks: long gap runs placed on the
kernels' band and window edges, repeats, and 4-symbol alphabets other than
ACGT.  Generators only -- no test functions, nothing here loads libnwk.so
(seqalign.pair_index and seqalign.moves_of are pure Python).

Every generator is deterministic (random.Random with the seeds below) and
returns (genes, ids, labels): the sequences, an explicit list of canonical
pair ids (pair (i, j), j < i, has genes[i] as rows and genes[j] as columns)
and one label per id for failure messages.  A block-family label starts with
"U run=<len>" or "L run=<len>": the one gap run the oracle's alignment of that
pair holds (tests/test_structured_inputs.py checks it does).
"""
import itertools
import random

import seqalign

SEED_BLOCK = 20260131
SEED_N = 20260132
SEED_LOW = 20260133

# gap-run lengths: one below, at and one above the walks' 32-key windows, 64-column
# tiles, 128-row tiles and 2048-row bands
A = (31, 32, 33, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049)
P_LEN = 2030        # the block starts on row / column 2031 and crosses 2048 for every a
EDGE = 2048         # a band edge of every kernel, and a 512-, 256-, 128-, 64- and 32-edge
EDGE_A = (33, 129)  # runs that end (len(P) = EDGE - a) or start (len(P) = EDGE) exactly on EDGE
CROSS = ((33, 2049), (64, 129), (2047, 2048))  # ins_a x ins_b pairs: one run of b - a

# The scorings the GPU tests run each family under (tests/test_gpu_structured.py); the CPU
# tests check the families' properties under the same ones.  The block family needs pxy > 0:
# with pxy = 0 it degenerates to one diagonal.
BLOCK_LINEAR = [(3, 2), (5, 1), (4, 2), (1, 1)]
BLOCK_AFFINE = [(3, 3, 1), (2, 4, 2), (9, 3, 2), (3, 0, 2)]  # (pxy, go, ge)
STRIP_LINEAR = [(3, 2), (5, 1)]
LOW_LINEAR = [(3, 2), (5, 1), (0, 2)]


def _rand(r, n, symbols):
    return bytes(r.choice(symbols) for _ in range(n))


def _block_family(r, p_len, q_len, a_values, edge, edge_a, cross, alphabet, n_in_q, lean):
    three, block = alphabet[:3], alphabet[3:4]
    P, Q = _rand(r, p_len, three), _rand(r, q_len, three)
    variants = [(plen, a, _rand(r, plen, three)) for a in edge_a for plen in (edge - a, edge)]
    if n_in_q:  # a fifth symbol, the same in every copy of Q
        q = bytearray(Q)
        for t in random.Random(SEED_N).sample(range(q_len), n_in_q):
            q[t] = ord("N")
        Q = bytes(q)
    B = P + Q
    genes = [B] + [P + block * a + Q for a in a_values] + [B]
    at = {a: 1 + t for t, a in enumerate(a_values)}
    last = len(genes) - 1
    ids, labels = [], []

    def pair(i, j, label):
        ids.append(seqalign.pair_index(i, j))
        labels.append(label)

    for a in a_values:
        pair(at[a], 0, "U run=%d ins_%d x B, len(P)=%d" % (a, a, p_len))
    for a in a_values:
        pair(last, at[a], "L run=%d B x ins_%d, len(P)=%d" % (a, a, p_len))
    for a, b in cross:
        if lean and b - a == 1:
            continue
        pair(at[b], at[a], "U run=%d ins_%d x ins_%d, len(P)=%d" % (b - a, b, a, p_len))
    for plen, a, Pv in variants:
        Bv, ins = Pv + Q, Pv + block * a + Q
        # lean: one orientation per variant, U for the first edge run length and L for the second
        want_u = not lean or a == edge_a[0]
        want_l = not lean or a != edge_a[0]
        base = len(genes)
        if want_u and want_l:
            genes += [Bv, ins, Bv]
        elif want_u:
            genes += [Bv, ins]
        else:
            genes += [ins, Bv]
        if want_u:
            pair(base + 1, base, "U run=%d ins_%d x B, len(P)=%d" % (a, a, plen))
        if want_l:
            pair(base + 2 if want_u else base + 1, base + 1 if want_u else base,
                 "L run=%d B x ins_%d, len(P)=%d" % (a, a, plen))
    return genes, ids, labels


def block_gaps(q_len=700, alphabet=b"ACGT", n_in_q=0):
    """B = P + Q against ins_a = P + (4th symbol) * a + Q, P and Q random over the
    first three symbols: for pxy > 0 the alignment is one gap run of exactly a
    (the block is the only place the 4th symbol occurs, so nothing in it can
    match), on rows 2031 .. 2030 + a (ins_a as rows: a U run) or on those columns
    (ins_a as columns: an L run).  Plus the runs that end or start exactly on
    row / column 2048, and three ins_a x ins_b pairs.

    The family of q_len = 2100 (4,130 columns and more: nw_align_strip's domain)
    has four times the cells, so it is lean: it leaves out the ins_2047 x ins_2048
    pair (a run of 1) and keeps one orientation per edge variant (a = 33 as U
    runs, a = 129 as L runs); every a, both orientations of the main family and
    both edge placements stay.  n_in_q > 0 writes that many 'N' into Q."""
    r = random.Random(SEED_BLOCK)
    return _block_family(r, P_LEN, q_len, A, EDGE, EDGE_A, CROSS, alphabet, n_in_q, lean=q_len > 1000)


def block_gaps_small(alphabet=b"ACGT"):
    """The block family scaled down for a pure-Python check: P = 60, Q = 40, a in (5, 33)."""
    r = random.Random(SEED_BLOCK + 1)
    return _block_family(r, 60, 40, (5, 33), 64, (), ((5, 33),), alphabet, 0, lean=False)


def _all_pairs(names):
    ids, labels = [], []
    for i in range(1, len(names)):
        for j in range(i):
            ids.append(seqalign.pair_index(i, j))
            labels.append("%s x %s" % (names[i], names[j]))
    return ids, labels


def _low(r, h1, h2, c, ac, ca, z, tail):
    Z = _rand(r, z, b"ACGT")
    named = [("A*%d" % h1, b"A" * h1), ("A*%d" % h2, b"A" * h2), ("C*%d" % c, b"C" * c),
             ("AC*%d" % ac, b"AC" * ac), ("CA*%d" % ca, b"CA" * ca), ("Z", Z), ("Z again", Z),
             ("Z[1:]", Z[1:]), ("Z[:-1]", Z[:-1]), ("A*%d+C*%d" % (h1, tail), b"A" * h1 + b"C" * tail),
             ("C*%d+A*%d" % (tail, h1), b"C" * tail + b"A" * h1)]
    ids, labels = _all_pairs([n for n, _ in named])
    return [g for _, g in named], ids, labels


def low_complexity():
    """Homopolymers, dinucleotide repeats, identical and shifted copies: every
    cell of A*n x A*m is a tie, Z x Z is a 4,100-cell pure diagonal over two band
    edges, A*n x C*m at (5, 1) is all gaps (a vertical run from (m, n) to row 0).
    All 55 pairs."""
    return _low(random.Random(SEED_LOW), 2049, 4100, 2100, 1100, 1075, 4100, 70)


def low_complexity_affine():
    """low_complexity() with the six pairs among A*2049, A*4100, C*2100, Z and Z
    again that involve A*4100, C*2100 or Z (the affine oracle keeps three
    matrices: all 55 pairs would take it too long)."""
    genes, _, _ = low_complexity()
    names = {0: "A*2049", 1: "A*4100", 2: "C*2100", 5: "Z", 6: "Z again"}
    pairs = [(1, 0), (2, 0), (2, 1), (5, 1), (5, 2), (6, 5)]
    return (genes, [seqalign.pair_index(i, j) for i, j in pairs],
            ["%s x %s" % (names[i], names[j]) for i, j in pairs])


def msa_sets():
    """Two sets for the progressive MSA, whose profile kernel works in 256-row
    bands: the block family with runs of 33, 129 and 257 between two copies of
    B, and repeats of 256 to 300 (no ids: the MSA takes the whole set)."""
    r = random.Random(SEED_BLOCK)
    P, Q = _rand(r, P_LEN, b"ACG"), _rand(r, 700, b"ACG")
    blocks = [P + Q] + [P + b"T" * a + Q for a in (33, 129, 257)] + [P + Q]
    repeats = [b"A" * 300, b"A" * 257, b"C" * 256, b"AC" * 128, b"CA" * 130]
    return {"block-33-129-257": blocks, "repeats-256-300": repeats}


def low_complexity_small():
    """low_complexity() scaled down for a pure-Python check: homopolymers of 30 to 40, Z = 70."""
    return _low(random.Random(SEED_LOW + 1), 31, 40, 33, 17, 16, 70, 9)


# 4-byte tables the block family is re-spelt in (translate): ACGT -> table
ALPHABETS = {
    "bytes-01-7f-80-ff": b"\x01\x7f\x80\xff",  # both ends of the signed and the unsigned byte range
    "aAcC": b"aAcC",                           # case differs by one bit
    "AC_G": b"AC_G",                           # '_' in the input: the trim bites, host finalize only
}
# fewer symbols: the block's symbol also occurs in P and Q (3), two symbols, one (every cell a tie)
FEWER_SYMBOLS = {"3-symbols": b"ACGC", "2-symbols": b"ACAC", "1-symbol": b"AAAA"}
N_IN_Q = 40  # the 5-symbol family: block_gaps(n_in_q=N_IN_Q)


def translate(genes, table):
    """genes with A, C, G, T re-spelt as table[0..3]; other bytes stay."""
    t = bytes.maketrans(b"ACGT", bytes(table))
    return [g.translate(t) for g in genes]


def sum_cells(genes, ids):
    return sum(len(genes[i]) * len(genes[j]) for i, j in map(seqalign.pair_ij, ids))


def walked_runs(a1, a2, m, n):
    """(D, U, L): the longest run of each move type among the walk-order moves
    of an alignment's rows (seqalign.moves_of: from (m, n) until a row or column
    is exhausted)."""
    best = {ord("D"): 0, ord("U"): 0, ord("L"): 0}
    for mv, grp in itertools.groupby(seqalign.moves_of(a1, a2, m, n)):
        best[mv] = max(best[mv], sum(1 for _ in grp))
    return best[ord("D")], best[ord("U")], best[ord("L")]


def gap_runs(a1, a2):
    """The maximal gap runs of an alignment's rows, front to back: [("U" | "L", length)]
    (U: '_' in the column sequence's row a2, L: '_' in a1)."""
    kinds = ("U" if c2 == 95 else "L" if c1 == 95 else "D" for c1, c2 in zip(a1, a2))
    return [(k, sum(1 for _ in grp)) for k, grp in itertools.groupby(kinds) if k != "D"]
