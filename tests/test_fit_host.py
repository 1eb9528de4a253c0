"""The restatement of the model-fitting rules (tests/_fit.py) on hand-made alignments, the bincode image of a fitted model, and the
host arithmetic the device results are compared with — no GPU."""
import hashlib
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from simmr_amd import model_io
from tests import _fit

E = _fit.encode3
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/fit_model_main.cpp over custom_model.hpp and fit_host.hpp, built with the sanitizers as tests/test_sam_sort_host.py builds its own"""
    exe = tmp_path_factory.mktemp("fit") / "fit_model_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           str(ROOT / "tests" / "fit_model_main.cpp")])
    return exe


def fitted_dict():
    rng = np.random.default_rng(4)
    n_ref, n_pos = 40, 9
    per = rng.integers(1, 6, n_ref)
    first = np.concatenate([[0], np.cumsum(per)]).astype(np.uint64)
    dens = rng.random((n_pos, 71))
    dens[3] = 0.0
    dens[3, 60] = 1.0
    return {"qual_density": dens, "kmer_ref": np.sort(rng.choice(1 << 21, n_ref, replace=False)).astype(np.uint32), "kmer_first": first,
            "pair_alt": rng.integers(0, 1 << 21, int(first[-1])).astype(np.uint32), "pair_prob": rng.random(int(first[-1])).astype(np.float32),
            "length_density": rng.random(6), "length_lo": np.arange(100, 160, 10, dtype=np.uint32), "length_hi": np.array([109, 119, 129, 139, 149, 151], dtype=np.uint32),
            "insert_density": rng.random(4), "insert_lo": np.arange(300, 380, 20, dtype=np.uint32), "insert_hi": np.arange(319, 399, 20, dtype=np.uint32),
            "k": 7, "insert_size_mean": 333.25, "insert_size_std": 17.5, "read_length_mean": 131.125, "read_length_std": 12.75, "is_long": 0,
            "length_bin_width": 10, "insert_bin_width": 20}


def test_loader_reads_what_the_writers_write_and_the_cpp_writer_writes_the_same_bytes(harness, tmp_path):
    """serialize_fitted -> parse_model (custom_model.hpp) -> serialize_model (fit_host.hpp): the loader accepts the image whole, sees
    the shape that went in, and the C++ writer gives model_io's bytes back; the same for the synthetic stand-ins"""
    m = fitted_dict()
    long_m = dict(m, is_long=1, insert_lo=np.zeros(0, dtype=np.uint32), insert_hi=np.zeros(0, dtype=np.uint32), insert_density=np.zeros(0))
    for name, image in (("fitted", model_io.serialize_fitted(m)), ("fitted_long", model_io.serialize_fitted(long_m)),
                        ("short", model_io.synthetic_short_model()), ("long", model_io.synthetic_long_model())):
        src, dst = tmp_path / f"{name}.bin", tmp_path / f"{name}.out"
        src.write_bytes(image)
        r = subprocess.run([str(harness), "roundtrip", str(src), str(dst)], capture_output=True, text=True)
        assert r.returncode == 0, (name, r.stdout, r.stderr)
        assert dst.read_bytes() == image, name
        if name.startswith("fitted"):
            shape = r.stdout.splitlines()
            f = shape[0].split()
            assert [int(x) for x in f[:10]] == [9, 7, 40, int(m["kmer_first"][-1]), int(name == "fitted_long"), int(name == "fitted"), 6, 10,
                                                4 if name == "fitted" else 0, 20 if name == "fitted" else 0], shape
            assert [float(x) for x in f[10:]] == [131.125, 12.75, 333.25, 17.5] and shape[1].split() == ["70", "71", "70"]
    (tmp_path / "cut.bin").write_bytes(model_io.serialize_fitted(m)[:-3])
    r = subprocess.run([str(harness), "roundtrip", str(tmp_path / "cut.bin"), str(tmp_path / "cut.out")], capture_output=True, text=True)
    assert r.returncode == 1 and r.stdout.startswith("ERR")


@pytest.mark.parametrize("clamp", [1, 0])
def test_cpp_bins_from_a_histogram_are_the_restatement_s(harness, tmp_path, clamp):
    """make_bins (fit_host.hpp, what simmr_fit_plan runs): n, mean, deviation, Freedman-Diaconis width from the cumulative histogram's
    quartiles, and the ranges, against tests/_fit.bins over the sorted list"""
    rng = np.random.default_rng(2)
    cases = [[150] * 7, [100, 100, 140, 180, 181], [5], rng.integers(90, 160, 1001).tolist(), rng.integers(200, 5000, 64).tolist(),
             (rng.gamma(4.0, 2000.0, 300).astype(int) + 1).clip(1, 65535).tolist(), [1, 2], [7, 7, 7, 9]]
    for xs in cases:
        vals, counts = np.unique(xs, return_counts=True)
        f = tmp_path / "h.txt"
        f.write_text("".join(f"{v} {c}\n" for v, c in zip(vals.tolist(), counts.tolist())))
        out = subprocess.run([str(harness), "bins", str(clamp), str(f)], capture_output=True, text=True, check=True).stdout.splitlines()
        n, mean, sd, width, point = out[0].split()
        want_width, want_ranges, _ = _fit.bins(sorted(xs), bool(clamp))
        assert int(n) == len(xs) and int(width) == want_width and int(point) == int(min(xs) == max(xs)), (xs[:8], out[0])
        assert [tuple(int(x) for x in line.split()) for line in out[1:]] == want_ranges, xs[:8]
        _fit.assert_close([float(mean), float(sd)], [_fit.mean([float(x) for x in xs]), _fit.std_deviation([float(x) for x in xs])], "mean, sd")


def test_writer_bytes_are_pinned():
    """serialize_model writes for the synthetic stand-ins what it wrote before it gained the bin-width keywords (hashes taken from the
    writer as it was)"""
    for image, want in ((model_io.synthetic_short_model(), "ab607bfbe4ee776b6a1960fbf4b1a7b680a1c42de8da16065d957bb55f929f16"),
                        (model_io.synthetic_long_model(), "39da91ea46b4195dc4c7c39bad9c3a5ee405a14ad976f3b2718897d5fa1fef34"),
                        (model_io.synthetic_long_model(deletion=True, kmer_size=5), "6917d9bdf9ec964ee30cbd5982543544a8d73695026da77aefb13dcbee402541")):
        assert hashlib.sha256(image).hexdigest() == want


def test_kmer_rule_on_hand_made_alignments():
    k = 3
    # unchanged: windows 0 .. L - k - 1 (the last one is left out), each adds 2 to (ref, ref)
    assert _fit.kmerize_alignment(k, b"ACGTA", b"ACGTA") == {(E(b"ACG"), E(b"ACG")): 2, (E(b"CGT"), E(b"CGT")): 2}
    # L = k: no window; L = k + 1: one
    assert _fit.kmerize_alignment(k, b"ACG", b"ACG") == {}
    assert _fit.kmerize_alignment(k, b"ACGT", b"ACGT") == {(E(b"ACG"), E(b"ACG")): 2}
    # a substitution: (ref, ref) and (ref, query) one each
    assert _fit.kmerize_alignment(k, b"ACGT", b"ATGT") == {(E(b"ACG"), E(b"ACG")): 1, (E(b"ACG"), E(b"ATG")): 1}
    # N in the query leaves and is appended again; an all-N query window is skipped
    assert _fit.kmerize_alignment(k, b"ACGT", b"ANGT") == {(E(b"ACG"), E(b"ACG")): 1, (E(b"ACG"), E(b"AGN")): 1}
    assert _fit.kmerize_alignment(k, b"ACGT", b"NNNT") == {}
    # a non-ACGT reference byte skips every window over it
    assert _fit.kmerize_alignment(k, b"ACNTACG", b"ACGTACG") == {(E(b"TAC"), E(b"TAC")): 2}
    # a gap in the query row (a deletion): the query k-mer is padded with N
    assert _fit.kmerize_alignment(k, b"ACGT", b"A-GT") == {(E(b"ACG"), E(b"ACG")): 1, (E(b"ACG"), E(b"AGN")): 1}
    # a gap in the reference row (an insertion): windows that start with it or hold it are skipped
    assert _fit.kmerize_alignment(k, b"A-CGTAC", b"ATCGTAC") == {(E(b"CGT"), E(b"CGT")): 2, (E(b"GTA"), E(b"GTA")): 2}
    # a written byte the encoder refuses
    assert _fit.kmerize_alignment(k, b"ACGT", b"ARGT") == {}


def test_vectorised_rule_is_the_plain_one():
    rng = np.random.default_rng(3)
    for k in (3, 7, 10):
        lens = [0, 1, k - 1, k, k + 1, 2 * k, 57, 16, 33]
        want_rows, have_rows, plain = [], [], {}
        for L in lens:
            w = np.frombuffer(b"ACGTN-", dtype=np.uint8)[rng.choice(6, L, p=[.24, .24, .24, .24, .02, .02])]
            h = w.copy()
            for j in rng.integers(0, max(L, 1), L // 6):
                h[j] = b"ACGTN-R"[rng.integers(0, 7)]
            want_rows.append(w)
            have_rows.append(h)
            _fit.kmerize_alignment(k, bytes(w.tolist()).replace(b"-", b"X"), bytes(h.tolist()), plain)  # (a staged '-' is a byte, not a gap)
        L = np.array(lens)
        j = np.concatenate([np.arange(n) for n in lens])
        got = _fit.kmerize_flat(k, np.concatenate(have_rows), np.concatenate(want_rows), j, np.repeat(L, L))
        assert got == plain and len(plain) > 3, k


def test_order_cut_and_probabilities():
    counts = {(5, 5): 10, (5, 9): 3, (5, 2): 3, (5, 7): 1, (1, 1): 2}
    got = _fit.kmer_probabilities(counts, 3)
    assert [r for r, _ in got] == [1, 5]
    assert [(a, c) for a, c, _ in got[1][1]] == [(5, 10), (2, 3), (9, 3)]  # count descending, ties by code; (7, 1) is cut
    assert got[1][1][0][2] == np.float32(10) / np.float32(17) and got[0][1][0][2] == np.float32(1.0)  # the total is the uncut one


def test_point_mass_rule():
    assert _fit.quality_density([60] * 9) == [1.0 if s == 60 else 0.0 for s in range(71)]
    assert _fit.quality_density([93]) == [0.0] * 70 + [1.0]
    d = _fit.quality_density([30, 31, 35])
    assert all(np.isfinite(d)) and abs(sum(d) - 1.0) < 1e-3 and len(d) == 71
    assert _fit.bins([150.0] * 7, True) == (10, [(150, 150)], [1.0])
    width, ranges, dens = _fit.bins([100, 100, 140, 180, 181], True)
    assert ranges[0][0] == 100 and ranges[-1][1] == 181 and len(dens) == len(ranges) and all(np.isfinite(dens))
    assert _fit.bins([100, 100, 140, 180, 181], False)[1][-1][1] >= 181  # insert bins: ends not clamped


def test_quartiles_from_a_histogram_are_those_of_the_sorted_list():
    rng = np.random.default_rng(1)
    for n in (1, 2, 3, 4, 5, 7, 8, 100, 1001):
        xs = sorted(rng.integers(90, 160, n).tolist())
        i1, i3 = _fit.quartile_indices(n)
        hist = np.bincount(xs)
        cum = np.cumsum(hist)
        from_hist = [int(np.searchsorted(cum, i, side="right")) for i in (i1, i3)]  # the first value whose cumulative count passes i
        assert from_hist == [xs[i1], xs[i3]], n


def test_bincode_image_of_a_fitted_model():
    """serialize_fitted writes what a reader of shared::encoding::ErrorModelParams expects: walked here field by field"""
    m = {"qual_density": np.full((2, 71), 1.0 / 71), "kmer_ref": np.array([0, 9], dtype=np.uint32), "kmer_first": np.array([0, 1, 3], dtype=np.uint64),
         "pair_alt": np.array([0, 9, 10], dtype=np.uint32), "pair_prob": np.array([1.0, 0.75, 0.25], dtype=np.float32),
         "length_density": np.array([0.5, 0.5]), "length_lo": np.array([100, 110], dtype=np.uint32), "length_hi": np.array([109, 115], dtype=np.uint32),
         "insert_density": np.array([1.0]), "insert_lo": np.array([300], dtype=np.uint32), "insert_hi": np.array([300], dtype=np.uint32),
         "k": 3, "insert_size_mean": 300.0, "insert_size_std": 0.0, "read_length_mean": 107.0, "read_length_std": 4.0, "is_long": 0,
         "length_bin_width": 10, "insert_bin_width": 10}
    b = model_io.serialize_fitted(m)
    at = 0

    def take(fmt):
        nonlocal at
        v = struct.unpack_from("<" + fmt, b, at)
        at += struct.calcsize("<" + fmt)
        return v if len(v) > 1 else v[0]

    def bins():
        num, width, nd = take("QQQ")
        dens = [take("d") for _ in range(nd)]
        ranges = [take("II") for _ in range(take("Q"))]
        return num, width, dens, ranges
    assert take("Q") == 1 and take("Q") == 2
    for _ in range(2):
        num, width, dens, ranges = bins()
        assert (num, width, len(dens)) == (70, 1, 71) and ranges == [(i, i) for i in range(70)]
    assert take("B") == 3 and take("Q") == 3 and take("Q") == 2
    assert take("I") == 0 and take("Q") == 1 and take("If") == (0, 1.0)
    assert take("I") == 9 and take("Q") == 2 and take("If") == (9, 0.75) and take("If") == (10, 0.25)
    assert take("dd") == (300.0, 0.0) and take("B") == 1 and bins() == (1, 10, [1.0], [(300, 300)])
    assert take("dd") == (107.0, 4.0) and bins() == (2, 10, [0.5, 0.5], [(100, 109), (110, 115)])
    assert take("B") == 0 and at == len(b)
    # the keyword arguments default to what the writer always wrote
    q = [([1.0], [(0, 0)])]
    assert model_io.serialize_model(q, ([1.0], [(5, 9)])) == model_io.serialize_model(q, ([1.0], [(5, 9)]), read_length_bin_width=1, insert_size_bin_width=1)


def test_cli_serialiser_writes_model_io_s_bytes(tmp_path):
    """write_fit_model (simmr_amd/host: what `simmr-hip --fit-model` writes) against model_io.serialize_fitted on one fitted dict"""
    import ctypes as C
    from simmr_amd import _abi
    subprocess.check_call(["make", "-s", "-C", str(ROOT / "simmr_amd" / "host"), "libsimmr_host.so"])
    lib = C.CDLL(str(ROOT / "simmr_amd" / "host" / "libsimmr_host.so"))
    lib.simmr_host_fit_model.restype = C.c_void_p
    lib.simmr_host_fit_model.argtypes = [C.POINTER(_abi.FitInfo), C.POINTER(_abi.FitOut), C.c_char_p]
    lib.simmr_host_free.argtypes = [C.c_void_p]
    m = fitted_dict()
    for variant in (m, dict(m, is_long=1, insert_lo=np.zeros(0, dtype=np.uint32), insert_hi=np.zeros(0, dtype=np.uint32), insert_density=np.zeros(0))):
        info = _abi.FitInfo(n_ref_kmers=len(variant["kmer_ref"]), n_pairs=len(variant["pair_alt"]), n_positions=len(variant["qual_density"]),
                            n_length_bins=len(variant["length_lo"]), n_insert_bins=len(variant["insert_lo"]),
                            length_bin_width=variant["length_bin_width"], insert_bin_width=variant["insert_bin_width"],
                            read_length_mean=variant["read_length_mean"], read_length_std=variant["read_length_std"],
                            insert_size_mean=variant["insert_size_mean"], insert_size_std=variant["insert_size_std"],
                            is_long=variant["is_long"], k=variant["k"], max_alt_kmers=20)
        keep = {n: np.ascontiguousarray(variant[n]) for n in _abi.FIT_COLUMNS if n in variant}
        cols = _abi.FitOut(**{n: a.ctypes.data for n, a in keep.items()})
        path = tmp_path / "m.bin"
        ptr = lib.simmr_host_fit_model(C.byref(info), C.byref(cols), str(path).encode())
        answer = C.string_at(ptr).decode()
        lib.simmr_host_free(ptr)
        assert answer == "OK" and path.read_bytes() == model_io.serialize_fitted(variant)


# ---- the cases of tests/test_gpu_fit_seams.py land where their builders say -----------------------------------------------------
def changed_and_all(k, host, r, oracle, genomes):
    """(windows, changed windows, distinct changed pairs) of read r by the plain rule on its two rows"""
    from tests import _fit_cases, _stats
    one = _fit_cases.rows(host, r, r + 1)
    _, _, _, _, have, want, _ = _stats.flat_reads(oracle, one, genomes)
    counts = _fit.kmerize_alignment(k, bytes(want.tolist()), bytes(have.tolist()))
    changed = {key: c for key, c in counts.items() if key[0] != key[1]}
    return sum(counts.values()) // 2, sum(changed.values()), len(changed)


def test_constants_parse():
    c = _fit.constants()
    assert list(c) == list(_fit.CONSTANTS) and all(isinstance(v, int) and v > 0 for v in c.values())
    assert c["FIT_LANES"] == 16 and c["FIT_MAX_L"] == _fit.MAX_L and c["FIT_WG_READS"] * c["FIT_LANES"] == 512
    assert c["FIT_LDS_K"] in range(3, 10) and c["FIT_MAX_PROBE"] & (c["FIT_MAX_PROBE"] - 1) == 0


def test_uniform_batches_scale_the_model_of_one_batch(oracle):
    """the scaled model of the flush case is tests/_fit.model of the same reads laid out in full, table for table"""
    from tests import _fit_cases as cases
    genomes = cases.host_genomes()
    for n_batches in (1, 3):
        u = cases.uniform_batches(oracle, genomes, n_batches)
        assert u.n_reads == cases.WG_READS * n_batches == len(u.host["start"])
        assert np.array_equal(u.host["seq"][:cases.WG_READS * cases.UNIFORM_L], u.host["seq"][-cases.WG_READS * cases.UNIFORM_L:])
        want = _fit.model(oracle, [u.host], genomes, 2, cases.QUAL_OFFSET, cases.UNIFORM_K, 20)
        assert set(want) == set(u.model)
        for name in want:
            assert np.array_equal(np.asarray(u.model[name]), np.asarray(want[name])), (name, n_batches)
            assert np.asarray(u.model[name]).dtype == np.asarray(want[name]).dtype, name
        _fit.assert_model(u.model, want, "uniform batches")
        assert want["length_hist"][cases.UNIFORM_L] == u.n_reads == want["insert_hist"][cases.UNIFORM_SPAN]
        assert (want["pair_alt"] != np.repeat(want["kmer_ref"], np.diff(want["kmer_first"].astype(np.int64)))).sum() > 8  # changed pairs
        assert (want["pair_alt"] >> np.uint32(3 * (cases.UNIFORM_K - 1))).max() == 4                                      # the written N


@pytest.mark.parametrize("k", [3, 7, 8, 10])
def test_seam_rows_land_on_both_sides_of_every_seam(oracle, k):
    from tests import _fit_cases as cases
    genomes = cases.host_genomes()
    case = cases.seam_rows(k)
    host = cases.reads_of(oracle, genomes, case.specs, np.random.default_rng(k))
    assert len(case.notes) == len(case.specs) == 3 * 2 * (2 * k + 1 + k + 3)
    for r, (spec, note) in enumerate(zip(case.specs, case.notes)):
        windows, changed, _ = changed_and_all(k, host, r, oracle, genomes)
        assert (windows, changed) == (note.windows, note.changed), (r, spec[:5])
    for E in cases.EDGES:
        at = sorted(p for n in case.notes if n.E == E and len(n.at) == 1 for p in n.at)
        assert at == sorted(2 * list(range(E - k, E + k)))
        sides = {cases.place(p)[:2] for p in at}
        assert sides == {cases.place(E - 1)[:2], cases.place(E)[:2]} and len(sides) == 2
        lengths = sorted(s[3] for s, n in zip(case.specs, case.notes) if n.E == E and not n.at)
        assert lengths == sorted(2 * list(range(E - 1, E + k + 2)))
    m = _fit.model(oracle, [host], genomes, 1, cases.QUAL_OFFSET, k, 20)
    assert len(m["pair_alt"]) > len(m["kmer_ref"]) and len(m["qual_hist"]) == case.n_positions
    assert [int(m["length_hist"][v]) for v in (255, 256, 257, 258)] == [2, 2, 2, 2]


def test_insert_pairs_and_full_table_land(oracle):
    from tests import _fit_cases as cases
    genomes = cases.host_genomes()
    case = cases.insert_pairs()
    host = cases.reads_of(oracle, genomes, case.specs, np.random.default_rng(1))
    assert sorted(_fit.insert_sizes(host, 2)) == case.kept and len(case.kept) == 2 * sum(s <= 5000 for s in case.spans)
    assert {1, 1023, 1024, 1025, 4999, 5000, 5001} <= set(case.spans) and max(case.spans) > 100_000
    assert any(a[4] != b[4] for a, b in zip(case.specs[0::2], case.specs[1::2])) and any(b[2] < a[2] for a, b in zip(case.specs[0::2], case.specs[1::2]))
    for D in (1, 2, 3, 8, 9, 257):
        t = cases.full_table(D)
        host = cases.reads_of(oracle, genomes, t.specs, np.random.default_rng(2))
        _, _, _, j, have, want, _ = _stats_flat(oracle, host, genomes)
        counts = _fit.kmerize_flat(t.k, have, want, j, np.full(j.size, t.k + 1))
        changed = {key: c for key, c in counts.items() if key[0] != key[1]}
        assert len(changed) == D == t.distinct and sorted(changed.values()) == sorted(t.times) and len({key[0] for key in counts}) == 1
        assert all(a >> (3 * (t.k - 1)) < 4 for _, a in changed)  # ACGT k-mers


def _stats_flat(oracle, host, genomes):
    from tests import _stats
    return _stats.flat_reads(oracle, host, genomes)
