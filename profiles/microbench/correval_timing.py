"""Timing of the scoring of a read error corrector's output (simmr_correval_truth_add + simmr_correval_truth_plan + simmr_correval_add +
simmr_correval_read): a synthetic truth SAM of `pairs` pairs of 150-bp reads (default 1 000 000: two million records) with one base in
a hundred substituted, as --sam writes it, and a synthetic corrected FASTQ of the same reads in which four errors in five are fixed and
one clean base in two thousand is damaged:
    python profiles/microbench/correval_timing.py [pairs]
The reads' bodies come from a pool of 4096, so that building the texts on the host stays a matter of seconds.  One warm-up pass at a
hundredth of the size, then ONE timed pass; prints the HIP-event time of each call (simmr_last_correval_ms), reads and bases per second,
and the bytes the scorer reads per base against the rate it reached.  On a shared machine run it under a time limit of its own:
    timeout -k 10 500 python profiles/microbench/correval_timing.py"""
import random
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

from simmr_amd import Engine  # noqa: E402

L, POOL = 150, 4096
COMP = str.maketrans("ACGT", "TGCA")


def pool(seed=7):
    rng = random.Random(seed)
    bodies = []
    for _ in range(POOL):
        ref = "".join(rng.choice("ACGT") for _ in range(L))
        seq = list(ref)
        for i in range(L):
            if rng.random() < 0.01:
                seq[i] = rng.choice([b for b in "ACGT" if b != ref[i]])
        qual = "".join(chr(33 + rng.choice((11, 25, 37, 40))) for _ in range(L))
        md, run = "", 0
        for a, b in zip(ref, seq):
            if a == b:
                run += 1
            else:
                md += "%d%s" % (run, a)
                run = 0
        md += str(run)
        rev = rng.random() < 0.5
        fixed = [ref[i] if seq[i] != ref[i] and rng.random() < 0.8 else rng.choice("ACGT") if rng.random() < 0.0005 else seq[i] for i in range(L)]
        seq, fixed = "".join(seq), "".join(fixed)
        nm = sum(a != b for a, b in zip(ref, seq))
        sam = "\tc1\t1000\t60\t%dM\t=\t1200\t350\t%s\t%s\tNM:i:%d\tMD:Z:%s\n" % (L, seq, qual, nm, md)
        fq = "\n%s\n+\n%s\n" % (fixed[::-1].translate(COMP) if rev else fixed, qual[::-1] if rev else qual)
        bodies.append((16 if rev else 0, sam, fq, nm))
    return bodies


def texts(pairs: int, bodies):
    sam, fq, errors = ["@HD\tVN:1.6\n@SQ\tSN:c1\tLN:5000000\n"], [], 0
    for p in range(pairs):
        for mate in (0, 1):
            flag, s, f, nm = bodies[(2 * p + mate) * 2654435761 % POOL]
            sam.append("%d\t%d%s" % (p, flag | (0x41, 0x81)[mate], s))
            fq.append("@%d/%d%s" % (p, mate + 1, f))
            errors += nm
    return np.frombuffer("".join(sam).encode(), dtype=np.uint8), np.frombuffer("".join(fq).encode(), dtype=np.uint8), errors


def one_pass(eng, pairs, bodies, report):
    import torch
    truth, reads, errors = texts(pairs, bodies)
    d_truth, d_reads = torch.from_numpy(truth.copy()).to(eng.device), torch.from_numpy(reads.copy()).to(eng.device)
    ev = eng.correction_eval_open(4)
    try:
        ev.truth_add(d_truth)
        t_truth = ev.last_ms()
        entries = ev.truth_plan()
        after_plan = ev.last_ms()
        ev.add(d_reads)
        after_add = ev.last_ms()
        c = ev.read()[0]
        t_read = ev.last_ms() - after_add
    finally:
        ev.close()
    t_plan, t_add = after_plan - t_truth, after_add - after_plan
    if report:
        bases = c["compared"]
        assert entries == 2 * pairs and c["scored"] == entries and c["fixed"] + c["left"] + c["miscorrected"] == errors
        per_base = (2 * len(reads) + 3 * bases) / bases   # the line index reads the text twice; the scorer the bases' byte and the two planes' bytes
        print(f"truth {entries} reads of {L} bp ({len(truth)} bytes, {errors} errors), corrected {c['records']} records ({len(reads)} bytes): "
              f"{c['fixed']} fixed, {c['left']} left, {c['damaged']} damaged, {c['kept']} kept")
        print(f"  truth_add {t_truth:.2f} ms ({entries / t_truth / 1e3:.1f} M reads/s, {len(truth) / t_truth / 1e6:.1f} GB/s of text), truth_plan {t_plan:.2f} ms, "
              f"add {t_add:.2f} ms ({entries / t_add / 1e3:.1f} M reads/s, {bases / t_add / 1e6:.2f} Gbase/s; at least {per_base:.2f} bytes read per base: "
              f"{per_base * bases / t_add / 1e6:.1f} GB/s), read {t_read:.2f} ms, together {t_truth + t_plan + t_add + t_read:.2f} ms; one run, untuned", flush=True)


def main():
    pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    bodies = pool()
    eng = Engine(0)
    one_pass(eng, max(pairs // 100, 1), bodies, False)   # warm-up
    one_pass(eng, pairs, bodies, True)
    eng.close()


if __name__ == "__main__":
    main()
