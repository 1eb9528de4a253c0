"""Timing of the scoring of a variant caller's VCF (simmr_vcfeval_truth_add + simmr_vcfeval_truth_plan + simmr_vcfeval_add): a
synthetic truth of 1 M sites on four contigs as --strain-vcf writes them, and a candidate of 1 M records made from it (every
third site dropped and replaced by a spurious one, every fifth with another allele, QUALs with fractions, a GT column on every
other record):
    python profiles/microbench/vcfeval_timing.py [sites] [repeats]
One warm-up pass, then `repeats` timed passes; prints per pass the HIP-event time of each call (simmr_last_vcfeval_ms) and the
text's bytes per second, then the medians, and beside them the time the plain Python model of tests/_vcfeval.py takes for the
first 100 000 records of either text (for orientation only).  On a shared machine run it under a time limit:
    timeout -k 10 300 python profiles/microbench/vcfeval_timing.py"""
import statistics
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

from simmr_amd import Engine  # noqa: E402
from tests import _vcfeval  # noqa: E402

NAMES = ["g0|c0", "g0|c1", "g1|c0", "g1|c1"]
BASES = "ACGT"


def texts(n):
    truth, cand = [], []
    for i in range(n):
        chrom, pos = NAMES[i % 4], 1000 + 20 * (i // 4)
        ref, alt = BASES[i % 4], BASES[(i + 1 + i // 4 % 3) % 4]
        ad_r, ad_a = i % 7, (i * 2654435761) % 61
        truth.append(f"{chrom}\t{pos}\t.\t{ref}\t{alt}\t.\t.\tDP={ad_r + ad_a};AD={ad_r},{ad_a};ADF={ad_r},{ad_a // 2};ADR=0,{ad_a - ad_a // 2};OTH=0\n")
        if i % 3 == 2:
            pos += 7   # a spurious site in place of the true one
        if i % 5 == 4:
            alt = next(b for b in BASES if b not in (ref, alt))
        tail = "\tGT:DP\t0/1:31" if i % 2 else ""
        cand.append(f"{chrom}\t{pos}\t.\t{ref}\t{alt}\t{i % 250}.{i % 10}\tPASS\tDP=31;MQ=60{tail}\n")
    return "".join(truth).encode(), "".join(cand).encode()


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    truth, cand = texts(n)
    eng = Engine(0)
    import torch
    import numpy as np
    d_truth = torch.from_numpy(np.frombuffer(truth, dtype=np.uint8).copy()).to(eng.device)
    d_cand = torch.from_numpy(np.frombuffer(cand, dtype=np.uint8).copy()).to(eng.device)
    ev = eng.vcf_eval_open(NAMES)
    rows = []
    for it in range(repeats + 1):
        ev.reset(NAMES)
        ev.truth_add(d_truth)
        t_add = ev.last_ms()
        entries = ev.truth_plan()
        t_plan = ev.last_ms() - t_add
        ev.add(d_cand)
        t_rec = ev.last_ms() - t_add - t_plan
        c = ev.read()[0]   # (the reduction over the entries is outside the spans)
        ok = entries == n and c["calls"] == n and c["sites_missed"] == n // 3 and c["correct"] == c["sites_found"]
        if it == 0:
            continue       # warm-up
        rows.append((t_add, t_plan, t_rec))
        print(f"pass {it}: {n} true sites ({len(truth)} bytes), {n} candidate records ({len(cand)} bytes): truth_add {t_add:.3f} ms "
              f"({len(truth) / t_add / 1e6:.2f} GB/s), truth_plan {t_plan:.3f} ms, add {t_rec:.3f} ms ({len(cand) / t_rec / 1e6:.2f} GB/s); "
              f"{c['correct']} correct, {c['wrong']} wrong; counts as made: {ok}", flush=True)
    med = [statistics.median(r[i] for r in rows) for i in range(3)]
    print(f"median of {repeats}: truth_add {med[0]:.3f} ms ({len(truth) / med[0] / 1e6:.2f} GB/s), truth_plan {med[1]:.3f} ms, add {med[2]:.3f} ms "
          f"({len(cand) / med[2] / 1e6:.2f} GB/s), together {sum(med):.3f} ms")
    ev.close()
    eng.close()
    k = min(n, 100_000)
    cut_t = b"\n".join(truth.split(b"\n")[:k]) + b"\n"
    cut_c = b"\n".join(cand.split(b"\n")[:k]) + b"\n"
    t0 = time.perf_counter()
    m = _vcfeval.Model(NAMES)
    m.truth_add(cut_t)
    m.truth_plan()
    t1 = time.perf_counter()
    m.add(cut_c)
    m.read()
    t2 = time.perf_counter()
    print(f"the Python model, one thread, the first {k} records of either text: truth {1e3 * (t1 - t0):.0f} ms, candidate {1e3 * (t2 - t1):.0f} ms "
          f"(for orientation only: no test depends on it; a single-thread C++ pass was not written)")


if __name__ == "__main__":
    main()
