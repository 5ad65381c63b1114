"""GPU parity of nw_align_col's paired tasks (csrc/nwk_col.hip, two words per
lane): one wave fills bands b and b + 1 of a pair as a 128-lane virtual wave,
word B 64 steps behind word A, the carries crossing from A's lane 63 to B's
lane 0 on the scalar unit.

Every case runs in two fresh child processes (NWK_COL_PAIR is read once per
process), NWK_COL_PAIR=1 and NWK_COL_PAIR=0, and compares penalties, problem
hashes and the answer hash three ways, all exactly: paired against the oracle,
unpaired against the oracle, paired against unpaired.

Shapes are the smallest at which the pairing can go wrong: two bands with the
second almost empty (m = 2049), exactly two (4096), a paired task plus a single
(4097), five bands (two paired tasks plus a single); columns narrower than
the 64 steps word B trails by (n = 5, 63), at it and just past it (64, 65, 97,
where the published granule index shifts by two halves) and an n that is no
multiple of 32 (150); single-band pairs in the same batch, so single and
paired tasks share one task list.
"""
import json
import os
import random
import subprocess
import sys

import pytest

import oracle
import seqalign

pytestmark = pytest.mark.gpu

ACGT = b"ACGT"
# both NP forms (pgap 2: four planes, pgap 1: two) and the SR extremes of each
SCORINGS = [(3, 2), (5, 1), (0, 2), (1, 1)]

_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import seqalign
cfg = json.loads(sys.stdin.read())
genes = [bytes.fromhex(g) for g in cfg["genes"]]
k = len(genes)
ids = np.asarray(cfg["ids"], dtype=np.int64) if cfg.get("ids") else np.arange(k * (k - 1) // 2, dtype=np.int64)
out = []
for pxy, pgap in cfg["scorings"]:
    with seqalign.Engine(device=0, kernel="nw_align_col", workspace_bytes=cfg.get("ws", 0)) as e:
        e.set_sequences(genes)
        pen, hs = e.align_pairs(ids, pxy, pgap)
        st = e.stats()
    out.append({"pen": [int(v) for v in pen], "hs": [x.tobytes().hex() for x in hs],
                "answer": seqalign.chain_hash(hs), "stats": st})
print(json.dumps(out))
"""


def _run(genes, scorings, ids=None, ws=0, **env):
    cfg = {"genes": [g.hex() for g in genes], "scorings": [list(s) for s in scorings], "ids": ids, "ws": ws}
    res = subprocess.run([sys.executable, "-c", _CHILD, os.path.dirname(seqalign.__file__)],
                         input=json.dumps(cfg).encode(), env=dict(os.environ, **env),
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    return json.loads(res.stdout.decode().strip().splitlines()[-1]), res.stderr.decode()


def _rand(r, n):
    return bytes(r.choice(ACGT) for _ in range(n))


_SHAPES = {}


def _shape_genes():
    """Narrow sequences on both sides of the many-band ones (the canonical pair
    (i, j), j < i, has genes[i] as rows), and swapped halves whose path runs
    ~1300 columns off the diagonal (it leaves a small storage window)."""
    if "genes" not in _SHAPES:
        r = random.Random(7071)
        narrow = (5, 63, 64, 65, 97, 150)
        genes = [_rand(r, n) for n in narrow]
        genes += [_rand(r, m) for m in (2049, 4096, 4097, 8200)]
        genes += [_rand(r, n) for n in narrow]
        P, Q = _rand(r, 1300), _rand(r, 1300)
        genes += [P + Q, Q + P]
        _SHAPES["genes"] = genes
    return _SHAPES["genes"]


def _shape_want(scoring):
    """The oracle's answer for the shape set, computed once per scoring."""
    if scoring not in _SHAPES:
        _SHAPES[scoring] = oracle.all_pairs(_shape_genes(), *scoring)
    return _SHAPES[scoring]


def _three_way(paired, single, want, what):
    oh, opens, ohs = want
    for name, o in (("paired", paired), ("unpaired", single)):
        assert o["stats"]["mode"] == 10, (what, name, o["stats"])
        bad = [(q, o["pen"][q], opens[q]) for q in range(len(opens)) if o["pen"][q] != opens[q]]
        assert not bad, "%s %s: penalties differ from the oracle (pair, got, want): %s" % (what, name, bad[:8])
        assert o["hs"] == ohs, "%s %s: problem hashes differ from the oracle" % (what, name)
        assert o["answer"] == oh, "%s %s: answer hash differs from the oracle" % (what, name)
    assert paired["pen"] == single["pen"] and paired["hs"] == single["hs"] and paired["answer"] == single["answer"], what
    assert paired["stats"]["col_paired_tasks"] > 0, (what, "NWK_COL_PAIR=1 ran no paired task", paired["stats"])
    assert single["stats"]["col_paired_tasks"] == 0, (what, single["stats"])


@pytest.mark.parametrize("storage", ["full", "windowed"])
def test_col_pair_band_counts_narrow_columns_mixed_batch(storage):
    """Band counts 1, 2, 3 and 5 in one batch against columns of 5 .. 150 and
    against each other, every scoring, with full storage and with a forced
    64-column window (NWK_COL_WIN, a workspace too small for full storage is
    not needed for it): the swapped halves leave the window, so their
    full-storage re-run goes through paired tasks too.  A clean run re-runs no
    pair for the fill-vs-walk guard: the end value sums both words."""
    genes = _shape_genes()
    env = {"NWK_COL_WIN": "64"} if storage == "windowed" else {"NWK_COL_WIN": "0"}
    paired, _ = _run(genes, SCORINGS, NWK_COL_PAIR="1", **env)
    single, _ = _run(genes, SCORINGS, NWK_COL_PAIR="0", **env)
    for sc, p, s in zip(SCORINGS, paired, single):
        what = "%s (pxy, pgap) = %s" % (storage, sc)
        _three_way(p, s, _shape_want(sc), what)
        for o in (p, s):
            assert o["stats"]["guard_checked"] >= len(o["pen"]) and o["stats"]["guard_reruns"] == 0, (what, o["stats"])
        if storage == "windowed":
            assert p["stats"]["window_retries"] > 0, (what, p["stats"])
        else:
            assert p["stats"]["window"] == 0 and p["stats"]["window_retries"] == 0, (what, p["stats"])


def test_col_pair_guard_catches_corrupt_cell_of_paired_fill():
    """NWK_DBG_CORRUPT=1 flips the stored D bit of cell (m, n) of slot 0, the
    batch's largest pair (4096 x 4000: one paired task): the walk's cost then
    differs from the fill's end value, which a paired task sums over both its
    words, and the pair is re-run once.  (The sequences end in a common tail,
    so the flipped cell's other moves cost more: no tie hides the flip.)"""
    r = random.Random(99)
    tail = _rand(r, 24)
    genes = [_rand(r, 3976) + tail, _rand(r, 4072) + tail, _rand(r, 76) + tail]
    want = oracle.all_pairs(genes, 3, 2)
    (p,), err = _run(genes, [(3, 2)], NWK_COL_PAIR="1", NWK_DBG_CORRUPT="1", NWK_GUARD_LOG="1")
    (s,), _ = _run(genes, [(3, 2)], NWK_COL_PAIR="0")
    _three_way(p, s, want, "corrupt")
    assert p["stats"]["guard_reruns"] == 1, (p["stats"], err[-1500:])
    assert "nwk guard: pair" in err
    assert s["stats"]["guard_reruns"] == 0


def test_col_pair_many_rounds_of_band_tasks_and_default_off():
    """A batch of over four rounds of band tasks per wave slot (8,704 two-band
    pairs of a few columns: 17,408 band tasks, so tasks of many pairs are in
    flight and the task queue drains while paired tasks run), paired and
    unpaired; and the default (no NWK_COL_PAIR) runs no paired task: pairing
    measured slower on the benchmark and is opt-in."""
    r = random.Random(515)
    narrow = [_rand(r, r.randint(5, 36)) for _ in range(64)]
    tall = [_rand(r, 2049 + (q % 7)) for q in range(136)]
    genes = narrow + tall
    ids = [seqalign.pair_index(64 + i, j) for i in range(len(tall)) for j in range(len(narrow))]
    pens, hs = [], []
    for i in range(len(tall)):
        for j in range(len(narrow)):
            p, a1, a2 = oracle.pair(tall[i], narrow[j], 3, 2)
            pens.append(p)
            hs.append(oracle.problem_hash(a1, a2))
    want = (oracle.chain(hs), pens, hs)
    (a,), _ = _run(genes, [(3, 2)], ids=ids, NWK_COL_PAIR="1", NWK_COL_WIN="0")
    (s,), _ = _run(genes, [(3, 2)], ids=ids, NWK_COL_PAIR="0", NWK_COL_WIN="0")
    _three_way(a, s, want, "many rounds")
    assert a["stats"]["col_paired_tasks"] == len(ids), a["stats"]
    assert a["stats"]["guard_reruns"] == 0
    env = {k: v for k, v in os.environ.items() if k != "NWK_COL_PAIR"}
    (d,), _ = _run_env(genes, ids, env, dict(NWK_COL_WIN="0"))
    assert d["stats"]["col_paired_tasks"] == 0 and d["pen"] == pens and d["hs"] == hs, d["stats"]


def _run_env(genes, ids, env, extra):
    cfg = {"genes": [g.hex() for g in genes], "scorings": [[3, 2]], "ids": ids, "ws": 0}
    res = subprocess.run([sys.executable, "-c", _CHILD, os.path.dirname(seqalign.__file__)],
                         input=json.dumps(cfg).encode(), env=dict(env, **extra),
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    return json.loads(res.stdout.decode().strip().splitlines()[-1]), res.stderr.decode()
