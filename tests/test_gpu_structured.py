"""GPU parity of every exported fill kernel and finalize path on structured
inputs (tests/structured.py): gap runs of exactly 31 .. 2049 that cross, end on
or start on row / column 2048 (a band edge of every kernel and a 512-, 256-,
128-, 64- and 32-edge), homopolymers and repeats (every cell a tie, a pure
diagonal of 4,100 cells, a vertical run of 2,100), and 4-symbol alphabets that
are not ACGT.  The rest of the suite draws uniform random ACGT or point-mutated
copies, whose alignments hold no interior gap run longer than 32.

Bar: penalties and per-pair problem hashes bit-exact against the oracle, whose
answer is computed once per (family, scoring) and shared by every kernel; each
test asserts the mode the run reports, so a fallback cannot pass for the
kernel under test.  tests/test_structured_inputs.py checks, without a GPU,
that the families keep the run lengths these tests are about.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import seqalign
import structured as S

pytestmark = pytest.mark.gpu

_FAMILY = {}
_WANT = {}


def family(name):
    """(genes, ids, labels) of a family by name, built once."""
    if name not in _FAMILY:
        if name == "block":
            _FAMILY[name] = S.block_gaps()
        elif name == "block-q2100":
            _FAMILY[name] = S.block_gaps(q_len=2100)
        elif name == "low":
            _FAMILY[name] = S.low_complexity()
        elif name == "low-affine":
            _FAMILY[name] = S.low_complexity_affine()
        elif name == "block-5-symbols":
            _FAMILY[name] = S.block_gaps(n_in_q=S.N_IN_Q)
        else:  # the block family re-spelt
            genes, ids, labels = family("block")
            table = dict(S.ALPHABETS, **S.FEWER_SYMBOLS)[name[len("block-"):]]
            _FAMILY[name] = (S.translate(genes, table), ids, labels)
    return _FAMILY[name]


def want(name, sc):
    """The oracle's (penalty, row 1, row 2, problem hash) per id of a family under a
    scoring ((pxy, pgap) or (pxy, go, ge)), computed once and never modified."""
    if (name, sc) not in _WANT:
        genes, ids, _ = family(name)
        out = []
        for pid in ids:
            i, j = seqalign.pair_ij(pid)
            pen, a1, a2 = oracle.pair(genes[i], genes[j], *sc) if len(sc) == 2 else oracle.pair_affine(
                genes[i], genes[j], *sc)
            out.append((pen, a1, a2, oracle.problem_hash(a1, a2)))
        _WANT[name, sc] = tuple(out)
    return _WANT[name, sc]


def compare(what, name, sc, pen, hashes_hex):
    labels = family(name)[2]
    w = want(name, sc)
    assert len(pen) == len(hashes_hex) == len(w), (what, name, sc)
    bad = ["%s: penalty got %d want %d, hash got %s.. want %s.." % (labels[q], pen[q], w[q][0], hashes_hex[q][:12],
                                                                    w[q][3][:12])
           for q in range(len(w)) if (int(pen[q]), hashes_hex[q]) != (w[q][0], w[q][3])]
    assert not bad, "%s, family %s, scoring %s: %d of %d pairs differ from the oracle:\n  %s" % (
        what, name, sc, len(bad), len(w), "\n  ".join(bad[:6]))


def _ids(name):
    return np.asarray(family(name)[1], dtype=np.int64)


def _poll_all(e, ids, pxy, pgap):
    """align_pairs through begin / poll / end: the polled records and end()'s must agree."""
    e.align_pairs_begin(ids, pxy, pgap)
    pen = np.zeros(len(ids), np.int32)
    hs = np.zeros((len(ids), 64), np.uint8)
    got = 0
    while got < len(ids):
        u, p_, h_ = e.align_pairs_poll(got)
        pen[got:u], hs[got:u] = p_, h_
        got = u
    pe, he = e.align_pairs_end()
    assert (pe == pen).all() and (he == hs).all(), "polled records differ from align_pairs_end's"
    return pen, hs


def run(name, sc, kernel, mode, streamed=False, **kw):
    """One family under one scoring on one engine: asserts the mode and the oracle's answer, returns the stats."""
    genes = family(name)[0]
    ids = _ids(name)
    with seqalign.Engine(device=0, kernel=kernel, **kw) as e:
        e.set_sequences(genes)
        if len(sc) == 3:
            pen, hs = e.align_pairs_affine(ids, *sc)
        elif streamed:
            pen, hs = _poll_all(e, ids, *sc)
        else:
            pen, hs = e.align_pairs(ids, *sc)
        st = e.stats()
    what = "kernel=%s %s" % (kernel, kw)
    if callable(mode):
        assert mode(st["mode"]), (what, name, sc, "mode", st["mode"])
    else:
        assert st["mode"] == mode, (what, name, sc, "mode %d, expected %d" % (st["mode"], mode))
    compare(what, name, sc, [int(v) for v in pen], [x.tobytes().hex() for x in hs])
    return st


def _packed_ok(pxy, pgap):
    """The packed integer kernels apply where the two profile bytes -2 pgap and
    pxy - 2 pgap have one sign (choose_plan); elsewhere a request for them runs nw_align."""
    return (-2 * pgap < 0) == (pxy - 2 * pgap < 0)


def linear_mode(kernel, sc):
    return {"nw_align_col": 10, "nw_align_bits": 8, "auto": 10, "nw_align": 0,
            "nw_align_pk": 4 if _packed_ok(*sc) else 0, "nw_align_pk2": 5 if _packed_ok(*sc) else 0}[kernel]


# --- linear kernels -------------------------------------------------------------------

LINEAR_KERNELS = ["nw_align_col", "nw_align_bits", "nw_align_pk", "nw_align_pk2", "nw_align", "auto"]
LINEAR_CASES = [("block", sc) for sc in S.BLOCK_LINEAR] + [("low", sc) for sc in S.LOW_LINEAR]


@pytest.mark.parametrize("kernel", LINEAR_KERNELS)
@pytest.mark.parametrize("name,sc", LINEAR_CASES, ids=["%s-%d/%d" % (n, *sc) for n, sc in LINEAR_CASES])
def test_linear_kernels_on_gap_runs_and_repeats(kernel, name, sc):
    """Every linear fill kernel and its walk: one gap run of 31 .. 2049 over the
    2048 edge per block pair (U and L), and the tie-heavy repeats."""
    run(name, sc, kernel, linear_mode(kernel, sc))


@pytest.mark.parametrize("sc", S.STRIP_LINEAR, ids=lambda sc: "%d/%d" % sc)
def test_strip_kernel_on_gap_runs(sc):
    """nw_align_strip (4,019 columns and more): the same runs across its 2048-row passes."""
    run("block-q2100", sc, "nw_align_strip", 9)


# --- nw_align_col and nw_align_bits: finalize paths -----------------------------------

@pytest.mark.parametrize("finalize", ["host", "device", "fused"])
@pytest.mark.parametrize("name,sc", [("block", (3, 2)), ("block", (5, 1)), ("low", (3, 2)), ("low", (5, 1))],
                         ids=["block-3/2", "block-5/1", "low-3/2", "low-5/1"])
def test_col_finalize_paths(finalize, name, sc):
    """nw_align_col with the host finalize, nw_rows + nw_hash after the launch, and the
    fused finalize streamed through align_pairs_begin / poll / end."""
    st = run(name, sc, "nw_align_col", 10, streamed=finalize == "fused", finalize=finalize)
    assert st["device_finalized"] == (0 if finalize == "host" else st["batches"]), st


@pytest.mark.parametrize("name,sc", [("block", (3, 2)), ("block", (5, 1)), ("low", (3, 2)), ("low", (5, 1))],
                         ids=["block-3/2", "block-5/1", "low-3/2", "low-5/1"])
def test_bits_fused_finalize(name, sc):
    st = run(name, sc, "nw_align_bits", 8, streamed=True, finalize="fused")
    assert st["device_finalized"] == st["batches"], st


# --- knobs read once per process: child processes -------------------------------------

_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import seqalign
cfg = json.loads(sys.stdin.read())
out = []
for job in cfg["jobs"]:
    genes = [bytes.fromhex(g) for g in cfg["genes"][job["family"]]]
    ids = np.asarray(cfg["ids"][job["family"]], dtype=np.int64)
    sc = job["scoring"]
    with seqalign.Engine(device=0, kernel=job["kernel"]) as e:
        e.set_sequences(genes)
        pen, hs = e.align_pairs(ids, *sc) if len(sc) == 2 else e.align_pairs_affine(ids, *sc)
        st = e.stats()
    out.append({"pen": [int(v) for v in pen], "hs": [x.tobytes().hex() for x in hs], "stats": st})
print(json.dumps(out))
"""


def run_child(jobs, **env):
    """jobs: [(family, scoring, kernel, mode)] in one fresh process under env; every job
    must report its mode and equal the oracle.  Returns the jobs' stats."""
    fams = sorted({j[0] for j in jobs})
    cfg = {"genes": {f: [g.hex() for g in family(f)[0]] for f in fams}, "ids": {f: list(family(f)[1]) for f in fams},
           "jobs": [{"family": f, "scoring": list(sc), "kernel": k} for f, sc, k, _ in jobs]}
    res = subprocess.run([sys.executable, "-c", _CHILD, os.path.dirname(seqalign.__file__)],
                         input=json.dumps(cfg).encode(), env=dict(os.environ, **env),
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    out = json.loads(res.stdout.decode().strip().splitlines()[-1])
    for (f, sc, k, mode), o in zip(jobs, out):
        what = "kernel=%s %s" % (k, env)
        assert o["stats"]["mode"] == mode, (what, f, sc, o["stats"])
        compare(what, f, sc, o["pen"], o["hs"])
    return [o["stats"] for o in out]


def _col_jobs(kernel="nw_align_col", mode=10):
    return [(f, sc, kernel, mode) for f in ("block", "low") for sc in ((3, 2), (5, 1))]


def test_col_paired_tasks():
    """NWK_COL_PAIR=1: two bands per wave, the runs crossing from word B's band into word A's."""
    for st in run_child(_col_jobs(), NWK_COL_PAIR="1"):
        assert st["col_paired_tasks"] > 0, st


def test_col_segmented_traceback():
    """NWK_COL_SEG=1: speculative segments started on the band edges the runs cross, end on and start on."""
    run_child(_col_jobs(), NWK_COL_SEG="1")


@pytest.mark.parametrize("env,kernel,mode", [({"NWK_COL_WIN": "64"}, "nw_align_col", 10),
                                             ({"NWK_BITS_WIN": "48"}, "nw_align_col", 10),
                                             ({"NWK_BITS_WIN": "48"}, "nw_align_bits", 8)],
                         ids=["col-NWK_COL_WIN=64", "col-NWK_BITS_WIN=48", "bits-NWK_BITS_WIN=48"])
def test_narrow_storage_window_reruns(env, kernel, mode):
    """A storage window narrower than the runs: the walk of a run of 65 and more leaves
    it, the pair re-runs with full storage, and the answer stays exact.  No pair
    re-runs for the fill-vs-walk guard."""
    jobs = _col_jobs(kernel, mode)
    for (f, sc, _, _), st in zip(jobs, run_child(jobs, **env)):
        assert st["guard_reruns"] == 0, (f, sc, st)
        if f == "block":
            assert st["window_retries"] > 0, (f, sc, st)


# --- linear-space traceback -----------------------------------------------------------

@pytest.mark.parametrize("g", [1, 2])
def test_linear_space_traceback_on_gap_runs(g):
    """Every pair through the linear-space path, g bands per recompute group: the
    runs cross the boundary row the groups are cut at."""
    st = run("block", (3, 2), "auto", 10, linear_space=g)
    assert st["linear_space_pairs"] == len(family("block")[1]), st


# --- affine ---------------------------------------------------------------------------

AFFINE_CASES = [("nw_align_gotoh", 11, sc) for sc in S.BLOCK_AFFINE] + [("nw_align_pk2", 7, (3, 3, 1)),
                                                                         ("nw_align", 3, (3, 3, 1))]


@pytest.mark.parametrize("name", ["block", "low-affine"])
@pytest.mark.parametrize("kernel,mode,sc", AFFINE_CASES, ids=["%s-%d/%d/%d" % (k, *sc) for k, _, sc in AFFINE_CASES])
def test_affine_kernels_on_gap_runs_and_repeats(name, kernel, mode, sc):
    """nw_align_gotoh (one ballot per D / U / L run), nw_align_pka and nw_align_affine:
    one affine gap of 31 .. 2049 per block pair; the homopolymer, C-against-A and
    identical pairs of the repeats."""
    run(name, sc, kernel, mode)


def test_gotoh_narrow_window_rerun():
    """NWK_BITS_WIN=40: the Gotoh walk leaves the stored blocks on the long runs and re-runs wider."""
    jobs = [(f, sc, "nw_align_gotoh", 11) for f in ("block", "low-affine") for sc in ((3, 3, 1), (2, 4, 2))]
    for (f, sc, _, _), st in zip(jobs, run_child(jobs, NWK_BITS_WIN="40")):
        if f == "block":
            assert st["window_retries"] > 0, (f, sc, st)


# --- alphabets ------------------------------------------------------------------------

COL_PATHS = [("nw_align_col", "auto"), ("auto", "auto"), ("nw_align_col", "host"), ("nw_align_col", "device"),
             ("nw_align_col", "fused")]


@pytest.mark.parametrize("kernel,finalize", COL_PATHS, ids=["%s-%s" % p for p in COL_PATHS])
@pytest.mark.parametrize("alphabet", sorted(S.ALPHABETS))
def test_four_symbol_alphabets_that_are_not_acgt(alphabet, kernel, finalize):
    """The block family re-spelt in bytes at both ends of the byte range, in two
    letters and their other case (one bit apart), and with '_' as a symbol: the
    bit-plane kernel must code any four bytes.  '_' in the input makes the trim
    bite, which only the host finalize does: the runtime must route it there
    even when the device or the fused finalize is asked for."""
    name = "block-" + alphabet
    for sc in ((3, 2), (5, 1)):
        st = run(name, sc, kernel, 10, streamed=finalize == "fused", finalize=finalize)
        if b"_" in S.ALPHABETS[alphabet] or finalize == "host":
            assert st["device_finalized"] == 0, st
        elif finalize != "auto":
            assert st["device_finalized"] == st["batches"], st


@pytest.mark.parametrize("symbols", sorted(S.FEWER_SYMBOLS))
def test_fewer_than_four_symbols(symbols):
    """Three symbols (the block's also occurs around it), two and one (every cell a
    tie): nw_align_col and nw_align_gotoh."""
    run("block-" + symbols, (3, 2), "nw_align_col", 10)
    run("block-" + symbols, (3, 3, 1), "nw_align_gotoh", 11)


def test_five_symbols_leave_the_bit_plane_kernels():
    """ACGT plus N: kernel="nw_align_col" must not run a two-plane kernel on it."""
    run("block-5-symbols", (3, 2), "nw_align_col", lambda mode: mode not in (8, 9, 10))


# --- alignment rows -------------------------------------------------------------------

def _row_pairs():
    out = []
    genes, _, labels = family("block")
    for kind in ("U", "L"):
        q = next(q for q, l in enumerate(labels) if l.startswith("%s run=2049 " % kind) and l.count("ins_") == 1)
        out.append(("block", q))
    _, _, labels = family("low-affine")
    out += [("low-affine", labels.index("Z again x Z")), ("low-affine", labels.index("A*4100 x A*2049"))]
    return out


def test_alignment_rows_of_long_runs():
    """get_minimum_penalty and get_minimum_penalty_affine: the rows of a U and an L
    run of 2049, of the identical pair and of homopolymer against homopolymer,
    byte for byte."""
    with seqalign.Engine(device=0) as e:
        for name, q in _row_pairs():
            genes, ids, labels = family(name)
            i, j = seqalign.pair_ij(ids[q])
            for sc, mode in (((3, 2), 10), ((3, 3, 1), 11)):
                fn = e.get_minimum_penalty if len(sc) == 2 else e.get_minimum_penalty_affine
                got = fn(genes[i], genes[j], *sc)
                assert e.stats()["mode"] == mode, (labels[q], sc, e.stats())
                w = want(name, sc)[q]
                assert got[0] == w[0], (name, labels[q], sc, "penalty got %d want %d" % (got[0], w[0]))
                assert got[1:] == w[1:3], (name, labels[q], sc, "rows differ", S.gap_runs(*got[1:])[:4],
                                           S.gap_runs(*w[1:3])[:4])


# --- MSA ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(S.msa_sets()))
def test_msa_on_gap_runs_and_repeats(name):
    """nwk_msa: gap runs of 33, 129 and 257 and repeats of 256 to 300 across
    nw_profile's 256-row bands; rows, length and sum-of-pairs score against the
    oracle's progressive MSA."""
    genes = S.msa_sets()[name]
    want_rows, want_s = oracle.msa(genes, 3, 2)
    with seqalign.Engine(device=0) as e:
        e.set_sequences(genes)
        rows, s = e.msa(3, 2)
    assert s == want_s, (name, "sum-of-pairs got %d want %d" % (s, want_s))
    assert [len(r) for r in rows] == [len(r) for r in want_rows], name
    bad = [q for q in range(len(genes)) if rows[q] != want_rows[q]]
    assert not bad, (name, "rows differ", bad)
    assert oracle.sop(rows, 3, 2) == s
