"""The structured input families (tests/structured.py) keep the properties the
GPU tests (tests/test_gpu_structured.py) rely on: one exact gap run per block
pair, walked runs longer than any band, at most four symbols, a fixed content
and a bounded size.  And the oracle itself, pinned on tie-heavy inputs by an
independent pure-Python restatement of the reference's traceback rule.

No GPU and no libnwk.so: the oracle (oracle/nw_oracle.c) and pure Python only.
"""
import hashlib

import pytest

import oracle
import seqalign
import structured as S


@pytest.fixture(scope="module", autouse=True)
def _built():
    oracle.build()


def _oracle_pair(x, y, sc):
    return oracle.pair(x, y, *sc) if len(sc) == 2 else oracle.pair_affine(x, y, *sc)


# --- exact runs -----------------------------------------------------------------------

EXACT = [(700, sc) for sc in S.BLOCK_LINEAR + S.BLOCK_AFFINE] + [(2100, sc) for sc in S.STRIP_LINEAR]


@pytest.mark.parametrize("q_len,sc", EXACT, ids=["q%d-%s" % (q, "/".join(map(str, sc))) for q, sc in EXACT])
def test_block_pairs_hold_one_exact_gap_run(q_len, sc):
    """Every labelled pair's oracle alignment has exactly one gap run, of the
    label's type and length, and costs exactly that run: nothing else in the
    alignment is a gap or a mismatch."""
    genes, ids, labels = S.block_gaps(q_len)
    for pid, label in zip(ids, labels):
        i, j = seqalign.pair_ij(pid)
        pen, a1, a2 = _oracle_pair(genes[i], genes[j], sc)
        kind, run = label.split()[0], int(label.split()[1][len("run="):])
        assert S.gap_runs(a1, a2) == [(kind, run)], (label, sc)
        assert pen == (run * sc[1] if len(sc) == 2 else sc[1] + run * sc[2]), (label, sc, pen)
        d, u, l = S.walked_runs(a1, a2, len(genes[i]), len(genes[j]))
        assert (u, l) == ((run, 0) if kind == "U" else (0, run)), (label, sc, d, u, l)


# --- long runs ------------------------------------------------------------------------

@pytest.mark.parametrize("pxy,pgap", [(3, 2), (5, 1)])
def test_low_complexity_reaches_runs_longer_than_a_band(pxy, pgap):
    genes, ids, _ = S.low_complexity()
    best = [0, 0, 0]
    for pid in ids:
        i, j = seqalign.pair_ij(pid)
        _, a1, a2 = oracle.pair(genes[i], genes[j], pxy, pgap)
        best = [max(b, v) for b, v in zip(best, S.walked_runs(a1, a2, len(genes[i]), len(genes[j])))]
    assert best[0] >= 4100, best
    if (pxy, pgap) == (5, 1):
        assert best[1] >= 2049, best


# --- shape ----------------------------------------------------------------------------

def _families():
    fam = {"block": S.block_gaps(), "block-q2100": S.block_gaps(q_len=2100), "low-complexity": S.low_complexity(),
           "block-5-symbols": S.block_gaps(n_in_q=S.N_IN_Q)}
    genes, ids, labels = fam["block"]
    for name, table in list(S.ALPHABETS.items()) + list(S.FEWER_SYMBOLS.items()):
        fam["block-" + name] = (S.translate(genes, table), ids, labels)
    return fam


FAMILIES = _families()

SHA256 = {
    "block": "910feff230fafd5f7c2271830f59cf5bd38edd915ea0955f6fed479d021f5c50",
    "block-q2100": "9ca212a825b28490ec44f51d3757b008266c59f77568ab0684e938b49b9271f1",
    "low-complexity": "35d9892a0eaf3c610e054c8d499a6d74b41ead61d81b4e4041f20cf120fd0ff4",
    "block-5-symbols": "3c0a9645ad4682e963c064003c5b028e89fa0dbc3cde9126424437bd2f64f2bd",
    "block-bytes-01-7f-80-ff": "3839b207b59ac948b079d82f67ba27487941a2392d1f9109cb92e741b4d0a3c6",
    "block-aAcC": "907adef190ab7dbebd5ff5adbdf5ea453d57dee48fe2b7dc66ca3cb15f9b5b5d",
    "block-AC_G": "ed2287403615431e8b4c0820c12f9b50a4b49bc73c612847a8945664abba6ab2",
    "block-3-symbols": "650b1dedd0bd24636d513561824d679b5a7d9ab5f096b18d1109f003688b4faf",
    "block-2-symbols": "6fd8fde992b6e08001d930c26028b66802b27be7f8dfd45c8b0d6527202468db",
    "block-1-symbol": "b3e83cd0b75cc8b74354c5eef6465473dc20e17f6ec53cc4c6d9f30d971c5886",
}
SYMBOLS = {"block-5-symbols": 5, "block-3-symbols": 3, "block-2-symbols": 2, "block-1-symbol": 1}


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_family_shape(name):
    """At most four distinct bytes (the bit-plane kernels' domain; the 5-symbol
    family exactly five, so it must leave them), fixed content, explicit
    canonical ids with a label each, and at most 6e8 cells over the ids: the
    size that keeps one GPU test, and the oracle's answer for it, at seconds."""
    genes, ids, labels = FAMILIES[name]
    assert len(set(b"".join(genes))) == SYMBOLS.get(name, 4)
    assert hashlib.sha256(b"\n".join(genes)).hexdigest() == SHA256[name], "the generator's output changed"
    k = len(genes)
    assert len(ids) == len(labels) == len(set(ids)) and all(0 <= p < k * (k - 1) // 2 for p in ids)
    assert S.sum_cells(genes, ids) <= 6e8


def test_block_family_places_every_run_on_the_edges():
    """The block of the main family starts on row / column 2031 and crosses 2048
    for every a; the edge variants end and start exactly on 2048; both
    orientations of every a are among the ids."""
    for q_len in (700, 2100):
        genes, ids, labels = S.block_gaps(q_len)
        seen = set()
        for pid, label in zip(ids, labels):
            i, j = seqalign.pair_ij(pid)
            kind, run = label.split()[0], int(label.split()[1][len("run="):])
            long_, short = (genes[i], genes[j]) if kind == "U" else (genes[j], genes[i])
            assert len(long_) - len(short) == run, label
            if label.count("ins_") == 2:
                continue  # ins x ins: the run is what the longer block has more
            start = long_.index(b"T")
            assert long_[start:start + run] == b"T" * run and long_[:start] + long_[start + run:] == short, label
            assert start < S.EDGE <= start + run or start == S.EDGE, label
            seen.add((kind, run, start))
        for a in S.A:
            assert ("U", a, S.P_LEN) in seen and ("L", a, S.P_LEN) in seen, (q_len, a)
        for a in S.EDGE_A:
            assert {s for k_, r_, s in seen if r_ == a} >= {S.P_LEN, S.EDGE - a, S.EDGE}, (q_len, a)
    # the strip family's columns are all in nw_align_strip's domain (n' = n + 32 rounded up to 64, >= 64 chunks)
    genes, ids, _ = S.block_gaps(q_len=2100)
    assert all((len(genes[seqalign.pair_ij(p)[1]]) + 32 + 63) // 64 >= 64 for p in ids)


# --- independent restatement ----------------------------------------------------------

def _fill_py(x, y, pxy, pgap):
    m, n = len(x), len(y)
    dp = [[j * pgap for j in range(n + 1)]] + [[i * pgap] + [0] * n for i in range(1, m + 1)]
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            dp[i][j] = dp[i - 1][j - 1] if x[i - 1] == y[j - 1] else min(
                dp[i - 1][j - 1] + pxy, dp[i - 1][j] + pgap, dp[i][j - 1] + pgap)
    return dp


def _walk_py(x, y, pxy, pgap, dp, order):
    """The reference's traceback (a diagonal move if the bytes match or
    dp[i-1][j-1] + pxy == dp[i][j], an up move if dp[i-1][j] + pgap == dp[i][j],
    a left move if dp[i][j-1] + pgap == dp[i][j]) with the three moves tried in
    `order`; "DUL" is the reference's.  Then its prefix and trim."""
    i, j, r1, r2 = len(x), len(y), [], []
    while i > 0 and j > 0:
        ok = {"D": x[i - 1] == y[j - 1] or dp[i - 1][j - 1] + pxy == dp[i][j],
              "U": dp[i - 1][j] + pgap == dp[i][j], "L": dp[i][j - 1] + pgap == dp[i][j]}
        mv = next(c for c in order if ok[c])
        r1.append(x[i - 1] if mv != "L" else 95)
        r2.append(y[j - 1] if mv != "U" else 95)
        i, j = i - (mv != "L"), j - (mv != "U")
    r1 += list(reversed(x[:i])) + [95] * j
    r2 += [95] * i + list(reversed(y[:j]))
    a1, a2 = bytes(reversed(r1)), bytes(reversed(r2))
    cut = max([t + 1 for t in range(len(a1)) if a1[t] == 95 and a2[t] == 95], default=0)
    return dp[len(x)][len(y)], a1[cut:], a2[cut:]


ORDERS = ["DUL", "DLU", "UDL", "ULD", "LDU", "LUD"]
PY_SCORINGS = [(3, 2), (5, 1), (4, 2), (1, 1)]


@pytest.fixture(scope="module")
def small_walks():
    """{(family, scoring, pair label): (the oracle's answer, {order: the restatement's})}"""
    out = {}
    for fam, (genes, ids, labels) in (("block", S.block_gaps_small()), ("low", S.low_complexity_small())):
        for sc in PY_SCORINGS:
            for pid, label in zip(ids, labels):
                i, j = seqalign.pair_ij(pid)
                x, y = genes[i], genes[j]
                dp = _fill_py(x, y, *sc)
                out[fam, sc, label] = (oracle.pair(x, y, *sc), {o: _walk_py(x, y, *sc, dp, o) for o in ORDERS})
    return out


def test_oracle_equals_python_restatement_on_structured_inputs(small_walks):
    """The oracle against a pure-Python Needleman-Wunsch with the reference's
    traceback rule, on scaled-down copies of both families (ties in nearly
    every cell of the low-complexity one)."""
    assert len(small_walks) == (5 + 55) * len(PY_SCORINGS)
    for key, (want, got) in small_walks.items():
        assert got["DUL"] == want, key


@pytest.mark.parametrize("order", ORDERS[1:])
def test_a_wrong_move_order_shows_on_low_complexity_pairs(small_walks, order):
    """Each of the five wrong tie-break orders gives another alignment than the
    oracle's on some low-complexity pair: these inputs tell the orders apart,
    which uniform random ACGT pairs rarely do."""
    caught = [key for key, (want, got) in small_walks.items() if key[0] == "low" and got[order] != want]
    assert caught, order


def test_block_family_has_no_ties(small_walks):
    """All six orders give the oracle's alignment on the scaled-down block
    family's B x ins pairs: a failure there is run mechanics, not tie order."""
    for key, (want, got) in small_walks.items():
        if key[0] == "block" and key[2].count("ins_") == 1:
            assert all(got[o] == want for o in ORDERS), key
