"""Fitting an error model from SAM text on the device (simmr_fit_add_sam, include/simmr_hip.h).  The central check is exact and
free: the SAM text the library writes for a run (Engine.sam / Engine.sam_sorted) must give the model of that run's columns
(Engine.fit_add), byte for byte.  Everything the round trip cannot show — gaps, clips, = / X, N and IUPAC letters, filters, text
geometry, malformed records — is hand-built and compared with the plain restatement of the rules (tests/_fit_sam.py)."""
import ctypes as C

import numpy as np
import pytest

from simmr_amd import MinimalLongErrorProfile, MinimalShortErrorProfile, SimmrError, _abi
from tests import _fit, _fit_sam
from tests.test_fit_sam_host import FILTER_LINES, filter_text, sam_line

pytestmark = pytest.mark.gpu
RNAMES = [(0, ["g0c0"]), (1, ["g1c0", "g1c1", "g1c2"])]
TILE = 4096  # bytes of a line-index tile


@pytest.fixture(scope="module")
def staged(engine):
    engine.stage_synthetic(0, [400_000], 1)
    engine.stage_synthetic(1, [300_000, 90_001, 30_017], 7)
    return engine


@pytest.fixture(params=[0, 16], ids=["compact", "slot16"])
def layout(request, engine):
    engine.set_read_slots(request.param)
    try:
        yield request.param
    finally:
        engine.set_read_slots(0)


def fit_columns(eng, shards, n_sets, k=7):
    eng.fit_reset(k, 20, 1 << 18)
    for s in shards:
        eng.fit_add(s, n_sets)
    return eng.fit_model()


def fit_sam(eng, texts, n_sets, k=7, max_alt=20):
    eng.fit_reset(k, max_alt, 1 << 18)
    for t in texts:
        eng.fit_add_sam(t, n_sets)
    return eng.fit_model()


def same_model(a, b, what):
    for name in _abi.FIT_COLUMNS:
        if a[name].dtype.kind in "ui":
            assert np.array_equal(a[name], b[name]), f"{what}: {name}"
    assert a["model_bytes"] == b["model_bytes"], what


def against_restatement(eng, texts, n_sets, k, what, max_alt=20):
    got = fit_sam(eng, texts, n_sets, k, max_alt)
    counts = eng.fit_sam_counts()
    want, want_counts = _fit_sam.fit(texts, n_sets, k, max_alt)
    assert counts == want_counts, what
    _fit.assert_model(got, want, what)
    return got, counts


# ---- 1: the round trip -----------------------------------------------------------------------------------------------------
def test_round_trip_short_pairs(staged, layout):
    eng = staged
    prof = MinimalShortErrorProfile(mean_phred_score=16, rng_mode=_abi.RNG_PHILOX).pod()
    shards = [eng.simulate_pe_reads_from_genome(g, prof, 300, 5 + g, qual_offset=33) for g in (0, 1)]
    for s in shards:
        h = s.to_host()
        st, en = h["start"].astype(np.int64), h["end"].astype(np.int64)
        span = np.maximum(np.maximum(st, en)[0::2], np.maximum(st, en)[1::2]) - np.minimum(np.minimum(st, en)[0::2], np.minimum(st, en)[1::2])
        assert span.max() <= _fit.MAX_INSERT
    want = fit_columns(eng, shards, 2)
    assert (want["pair_alt"] != np.repeat(want["kmer_ref"], np.diff(want["kmer_first"].astype(np.int64)))).sum() > 100  # changed windows
    texts = [eng.sam(s, RNAMES, True) for s in shards]
    got = fit_sam(eng, texts, 2)
    same_model(got, want, "SAM text in read order")
    c = eng.fit_sam_counts()
    n = sum(s.n_reads for s in shards)
    assert c["records"] == c["taken_quality"] == c["taken_alignment"] == n and c["lines"] == n and got["n_inserts"] == n
    same_model(fit_sam(eng, [eng.sam_sorted(s, RNAMES, True) for s in shards], 2), want, "SAM text in coordinate order")
    # bytes copied up instead of a tensor: the same
    same_model(fit_sam(eng, [t.cpu().numpy().tobytes() for t in texts], 2), want, "SAM text as bytes")


def test_round_trip_long_reads(staged, layout):
    eng = staged
    lp = MinimalLongErrorProfile(gamma_mean=600.0, gamma_std=400.0, length_mode=_abi.LEN_PER_READ, rng_mode=_abi.RNG_PHILOX).pod()
    dev = eng.simulate_long_reads([1, 0], [60, 40], lp, 3, qual_offset=33)
    want = fit_columns(eng, [dev], 1, k=8)
    assert want["n_positions"] > 512 and want["is_long"]
    same_model(fit_sam(eng, [eng.sam(dev, RNAMES, False)], 1, k=8), want, "minimal-long, read order")
    same_model(fit_sam(eng, [eng.sam_sorted(dev, RNAMES, False)], 1, k=8), want, "minimal-long, coordinate order")


# ---- 2: hand-built records ---------------------------------------------------------------------------------------------------
def record(ref, qry, flag=0, eqx=False, clips=(0, 0, 0, 0), qual=None, rng=None, **kw):
    """the SAM line of two aligned rows ('-' for a gap): CIGAR, MD and SEQ made here, clips = (H, S, S, H) around them"""
    assert len(ref) == len(qry)
    ops, md, run, in_del = [], "", 0, False
    for r, q in zip(ref, qry):
        if r == "-":
            ops.append("I")
            continue
        if q == "-":
            if not in_del:
                md += f"{run}^"
                run, in_del = 0, True
            md += r
            ops.append("D")
            continue
        in_del = False
        ops.append(("=" if r == q else "X") if eqx else "M")
        if r == q:
            run += 1
        else:
            md += f"{run}{r}"
            run = 0
    md += str(run)
    h5, s5, s3, h3 = clips
    runs = [("H", h5), ("S", s5)]
    for op in ops:
        if runs[-1][0] == op:
            runs[-1] = (op, runs[-1][1] + 1)
        else:
            runs.append((op, 1))
    runs += [("S", s3), ("H", h3)]
    cigar = "".join(f"{n}{op}" for op, n in runs if n)
    seq = "T" * s5 + "".join(q for q in qry if q != "-") + "G" * s3
    if qual is None:
        qual = "".join(chr(33 + int(v)) for v in (rng or np.random.default_rng(len(seq))).integers(0, 94, len(seq)))
    return sam_line(seq, cigar, md, flag=flag, qual=qual, **kw)


def random_rows(rng, n, p_sub=0.1, p_ins=0.08, p_del=0.08):
    ref, qry = [], []
    for _ in range(n):
        b = "ACGT"[rng.integers(0, 4)]
        u = rng.random()
        if u < p_ins:
            ref.append("-"), qry.append(b)
        elif u < p_ins + p_del:
            ref.append(b), qry.append("-")
        elif u < p_ins + p_del + p_sub:
            ref.append(b), qry.append("ACGT"[("ACGT".index(b) + 1 + rng.integers(0, 3)) % 4])
        else:
            ref.append(b), qry.append(b)
    return "".join(ref), "".join(qry)


def hand_built(k):
    rng = np.random.default_rng(100 + k)
    base = "".join("ACGT"[i] for i in rng.integers(0, 4, 4 * k + 8))
    n = len(base)
    lines = []
    for flag in (0, 16):
        lines += [record("-" + base, "G" + base[:-1] + "-", flag=flag)]                                     # I first, D last
        lines += [record(base[0] + base[1:] + "-", "-" + base[1:] + "C", flag=flag)]                      # D first, I last
        lines += [record(base[:k - 1] + "-" + base[k - 1:], base[:k - 1] + "A" + base[k - 1:k] + "-" + base[k + 1:], flag=flag)]  # across a window edge
        lines += [record(base[:k], base[:k], flag=flag), record(base[:k + 1], base[:k] + "A", flag=flag)]  # zero and one window
        lines += [record(base, base[:5] + "N" + base[6:], flag=flag, clips=(3, 4, 0, 0)), record(base, base, flag=flag, clips=(0, 0, 5, 2)),
                  record(base, base, flag=flag, clips=(1, 2, 3, 4))]
        lines += [record(*random_rows(rng, 3 * k + 5), flag=flag, eqx=True)]
        lines += [record("R" + base[1:k + 2] + "N" + base[k + 3:], base[:n // 2] + "N" + base[n // 2 + 1:], flag=flag)]  # IUPAC and N in MD, N in SEQ
        lines += [record(*random_rows(rng, m), flag=flag) for m in (17, 33, 255, 257, 700)]
        lines += [record(base[:12], base[:12], flag=flag, qual="!\"#$%&'()*+,")]                           # an asymmetric QUAL
    # >= 300 CIGAR runs and >= 300 MD runs: I, M, D, X in turn over 1400 columns
    ref, qry = [], []
    for i in range(350):
        b = "ACGT"[rng.integers(0, 4)]
        c = "ACGT"[("ACGT".index(b) + 1) % 4]
        ref += ["-", b, b, b]
        qry += [c, b, "-", c]
    lines += [record("".join(ref), "".join(qry), flag=f) for f in (0, 16)]
    assert lines[-1].split(b"\t")[5].count(b"I") >= 300 and lines[-1].split(b"\t")[-1].count(b"^") >= 300
    return b"".join(lines)


@pytest.mark.parametrize("k", [3, 7, 10])
def test_hand_built_records(engine, k):
    text = hand_built(k)
    got, counts = against_restatement(engine, [text], 1, k, f"hand-built records, k {k}", max_alt=5)
    assert counts["taken_alignment"] == counts["records"] and got["n_pairs"] > got["n_ref_kmers"] > 0
    assert (got["pair_alt"] >> np.uint32(3 * (k - 1))).max() == 4  # an N-padded alternate: a gap inside a window


# ---- 3: text geometry -----------------------------------------------------------------------------------------------------------
def test_text_geometry(engine):
    rng = np.random.default_rng(9)
    a, b = record(*random_rows(rng, 80)), record(*random_rows(rng, 120), flag=16)
    long_line = record(*random_rows(rng, 5000))                      # longer than two tiles
    assert len(long_line) > 2 * TILE + 100
    pad = b"@CO\t" + b"x" * (TILE - 1 - 5) + b"\n"                   # the next line starts on the tile's last byte
    assert len(pad) == TILE - 1
    text = pad + a + b"\n\n" + b"@CO\tbetween\n" + long_line + b"\n" + b + a.rstrip(b"\n")
    assert text[TILE - 1:TILE + 1] == a[:2] and not text.endswith(b"\n")
    _, counts = against_restatement(engine, [text], 1, 7, "text geometry")
    assert counts["lines"] == 6 and counts["header_lines"] == 2 and counts["taken_alignment"] == 4
    # only header lines; nothing at all
    engine.fit_reset(7, 20, 1000)
    engine.fit_add_sam(b"@HD\tVN:1.6\n@SQ\tSN:c0\tLN:5\n", 2)
    engine.fit_add_sam(b"", 2)
    c = engine.fit_sam_counts()
    assert c["lines"] == c["header_lines"] == 2 and sum(c.values()) == 4


# ---- 4: filters ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_sets", [1, 2])
def test_filters(engine, n_sets):
    got, counts = against_restatement(engine, [filter_text()], n_sets, 3, f"filters, {n_sets} sets")
    assert counts["skip_too_long"] == 1 and got["n_positions"] == _fit.MAX_L and got["length_hist"][_fit.MAX_L] == 1  # 65536 bases left out, 65535 taken
    if n_sets == 2:
        for name, _ in FILTER_LINES:
            assert counts[name] >= 1, name
        assert {name for name, _ in FILTER_LINES} == {n for n in _fit_sam.COUNTS if n.startswith("skip_")} | {"taken_alignment"}


# ---- 5: split invariance -------------------------------------------------------------------------------------------------------
def test_one_add_against_three(engine):
    text = hand_built(7)
    lines = text.splitlines(keepends=True)
    whole = fit_sam(engine, [text], 1)
    parts = fit_sam(engine, [b"".join(lines[:1]), b"".join(lines[1:9]), b"".join(lines[9:])], 1)
    same_model(parts, whole, "three adds")


def test_columns_and_sam_mixed(staged):
    eng = staged
    prof = MinimalShortErrorProfile(mean_phred_score=14, rng_mode=_abi.RNG_PHILOX).pod()
    whole = eng.simulate_pe_reads_from_genome(1, prof, 400, 9, qual_offset=33)
    first, second = (eng.simulate_pe_reads_from_genome(1, prof, 400, 9, first=f, count=c, qual_offset=33) for f, c in ((0, 150), (150, 250)))
    want = fit_columns(eng, [whole], 2)
    eng.fit_reset(7, 20, 1 << 18)
    eng.fit_add(first, 2)
    eng.fit_add_sam(eng.sam(second, RNAMES, True), 2)
    same_model(eng.fit_model(), want, "a columns add and a SAM add")


# ---- 6: errors -----------------------------------------------------------------------------------------------------------------
GOOD = sam_line("ACGTACGTAC", "10M", "10")
MALFORMED = {
    "10 fields": b"r\t0\tc0\t1\t60\t4M\t*\t0\t0\tACGT\n",
    "FLAG": GOOD.replace(b"r\t0\t", b"r\t0x\t"),
    "CIGAR": sam_line("ACGTACGTAC", "10", "10"),
    "QUAL length": sam_line("ACGTACGTAC", "10M", "10", qual="IIIIIIIII"),
    "QUAL byte": sam_line("ACGTACGTAC", "10M", "10", qual="IIII IIIII"),
}


@pytest.mark.parametrize("what", list(MALFORMED))
def test_malformed_record(engine, what):
    info = _abi.FitInfo()
    engine.fit_reset(7, 20, 1000)
    engine.fit_add_sam(GOOD + MALFORMED[what] + GOOD, 2)  # returns: the add only enqueues
    assert engine.lib.simmr_fit_plan(engine._h, C.byref(info)) == _abi.EINVAL and b"malformed" in engine.lib.simmr_last_error(engine._h)
    with pytest.raises(_fit_sam.Malformed):
        _fit_sam.fit([MALFORMED[what]], 2, 7, 20)
    engine.fit_add_sam(GOOD, 2)  # sticky until the reset
    with pytest.raises(SimmrError) as ei:
        engine.fit_model()
    assert ei.value.code == _abi.EINVAL
    assert fit_sam(engine, [GOOD], 2)["n_reads"] == 1


def test_argument_and_state_errors(engine):
    import torch
    from simmr_amd.engine import Engine
    lib, h = engine.lib, engine._h
    text = torch.from_numpy(np.frombuffer(GOOD, dtype=np.uint8).copy()).to(engine.device)
    engine.fit_reset(7, 20, 1000)
    for n_sets in (0, 3):
        assert lib.simmr_fit_add_sam(h, C.c_void_p(text.data_ptr()), text.numel(), n_sets) == _abi.EINVAL
    assert lib.simmr_fit_add_sam(h, None, 5, 2) == _abi.EINVAL
    assert lib.simmr_fit_add_sam(h, None, 0, 2) == 0
    fresh = Engine(0)
    try:
        assert fresh.lib.simmr_fit_add_sam(fresh._h, C.c_void_p(text.data_ptr()), text.numel(), 2) == _abi.ESTATE
        assert fresh.lib.simmr_fit_sam_counts_read(fresh._h, C.byref(_abi.FitSamCounts())) == _abi.ESTATE
    finally:
        fresh.close()
