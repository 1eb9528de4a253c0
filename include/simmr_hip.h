/*
 * simmr_hip.h — C ABI of the MI355X-native simmr hot path (libsimmr_hip.so).
 *
 * This is the drop-in boundary for the per-read sampling / mutation path of
 * genomicsoup/simmr.  The reference has no FFI: the seam is the call made once
 * per run from simmr/src/main.rs:180-186 into
 *     simulate::simulate_pe_reads      (simmr/src/simulate.rs:110-150)
 *     simulate::simulate_long_reads    (simmr/src/simulate.rs:323-406)
 * parameterised by the two trait objects
 *     ErrorProfile      (simmr/src/error_profiles/base.rs:6-32)
 *     AbundanceProfile  (simmr/src/abundance_profiles/base.rs:10-69).
 * Every entry point below names the reference interface it replaces.
 *
 * Conventions
 *   - plain C, no exceptions / unwinding across the boundary;
 *   - every function returns 0 (SIMMR_OK) or a negative errno-style code and
 *     simmr_last_error() gives the message (reference: Result<_, String>,
 *     simulate.rs:165-170,205-210);
 *   - one engine == one GPU == one host thread (not thread-safe), matching
 *     the single-threaded reference;
 *   - output buffers are caller-owned DEVICE pointers (hipMalloc / torch);
 *     the plan step reports the sizes needed (the reference returns owned
 *     Vec<SimulatedRead>, simulate.rs:119).
 *   - there is NO CPU fallback: without a gfx950 device every compute entry
 *     point fails with SIMMR_ENODEV.
 */
#ifndef SIMMR_HIP_H
#define SIMMR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIMMR_ABI_VERSION 1

/* status codes (negative errno values) */
#define SIMMR_OK 0
#define SIMMR_EINVAL (-22)  /* bad argument                                   */
#define SIMMR_ENOMEM (-12)  /* device/host allocation failed                  */
#define SIMMR_ENODEV (-19)  /* no usable gfx950 device / HIP runtime error    */
#define SIMMR_ERANGE (-34)  /* output capacity too small / value out of range */
#define SIMMR_ESTATE (-1)   /* call order violated (emit before plan, ...)    */
#define SIMMR_ENOTSUP (-95) /* valid request this library leaves to the host
                               (simmr_fastq_plan: see there)                  */
#define SIMMR_EGENOME (-61) /* genome unusable (reference: Err(String) at
                               simulate.rs:220-225 / infinite loop at :370)   */

/* ErrorProfile implementations, reference cli.rs:62-70 + error_profiles/mod.rs */
enum simmr_profile_kind {
  SIMMR_PERFECT_SHORT = 0, /* error_profiles/perfect_short.rs */
  SIMMR_MINIMAL_SHORT = 1, /* error_profiles/minimal_short.rs */
  SIMMR_PERFECT_LONG = 2,  /* error_profiles/perfect_long.rs  */
  SIMMR_MINIMAL_LONG = 3,  /* error_profiles/minimal_long.rs  */
  SIMMR_CUSTOM = 4         /* error_profiles/custom_short.rs  */
};

/* Which generator feeds the per-base draws.
 * REFERENCE: the reference's own streams — rand 0.8.5 StdRng (ChaCha12 keyed
 *   by PCG32 seed expansion) consumed exactly as simulate.rs / the profiles
 *   consume them.  Output is bit-identical to the reference for everything the
 *   reference itself makes deterministic under --seed.
 * PHILOX: counter-based Philox4x32-10 (Random123 constants) keyed by the read's Phred seed (key = its low and high
 *   words).  Specification, version 3 — stated in DESIGN.md section 4, restated independently in oracle/philox.c, which
 *   the kernels are compared with bit for bit:
 *     a base draws its Phred score q and its substitution s (0 = none, 1..3 = "ACGT"[(code + s) & 3]) TOGETHER from
 *     their joint law over the 1024 outcomes o = q | s << 8;
 *     level 1: 24 bits per base.  The 16 bases of group g = b >> 4 share the 384 bits of the three calls with counters
 *       (3g + {0, 1, 2}, 0, 0x73696D6D, 0x72000003) ('simm', 'r', version 3); base b takes bits [24 (b & 15), +24) = F;
 *       column F >> 14 of a 1024-column alias table (integer Vose construction over the 2^24 cells), fraction
 *       F & 0x3fff against the column's threshold in 16384ths;
 *     level 2, only for the E of 2^24 cells (E = 118 at mean Phred 30) that the integer split leaves over: counter
 *       (b >> 2, 1, 0x73696D6D, 0x72000003), word b & 3, a 1024-column alias table over the residual law with 22-bit
 *       thresholds.
 *   In rocRAND's terms (the library north_star names; tests/test_oracle_kat.py runs rocRAND's own engine class against
 *   the specification): a read's draws are the stream of rocrand_state_philox4x32_10 after
 *   rocrand_init(seed = the read's Phred seed, subsequence = 0x7200000373696D6D, offset = 4 * (c0 | c1 << 32), &state)
 *   — level 1 reads it from offset 4 * 3g (twelve consecutive outputs per group), level 2 at offset
 *   4 * ((b >> 2) | 1 << 32).  The kernels compute the same words with a hand-written round (two v_mad_u64_u32 and two
 *   v_bitop3_b32) rather than through the library's state object.
 *   Every profile with per-base draws: minimal-short, minimal-long, perfect-long as above, and the long-read path of a
 *   custom model (SIMMR_CUSTOM with an is_long model), whose base-by-base draws are those of the k-mer splice
 *   (simulate_errors, custom_short.rs:455-516; its qualities use a handful of words per read and stay the reference's):
 *     (specification of the splice's draws, version 2 — version 1 took two words per position and was never released)
 *     the alternate of the k-mer visited at position i is drawn from ONE word, X = word i & 3 of the block with
 *     key = the read's seed and counter (i >> 2, 2, 0x73696D6D, 0x72000003), in two levels over the reference's law
 *     P(alternate j) = w_j / sum(w):
 *       level 1, X >> 8 < T24 -> the k-mer stays what it is, with T24 = 2^24 - 2^e, 2^e the smallest power of two
 *         (1 <= e <= 24) of 2^24ths that holds 1 - P(self); a k-mer with an N has no "self": e = 24, T24 = 0;
 *       level 2 otherwise: Z = (X - (T24 << 8)) << (24 - e) is a full word again, m = Z * n (64 bits), column
 *         c = m >> 32 of an n-column alias table (Vose, f64, sums in list order) with thresholds in 2^24ths against
 *         (m & 0xffffffff) >> 8, over the residual law r_j = (p_j - [j is self] (T24 / 2^24) p_j / p_s) / (1 - T24 / 2^24).
 *     (oracle/custom.c: ctr_splice_tables / orc_custom_simulate_errors_philox; the paired-end path of a custom model
 *     has no base-by-base draws and refuses the mode.)
 *   Positions, lengths and seeds still come from the reference's streams.  Statistical tolerance only (BASELINE.json
 *   north_star): the law is the reference's (minimal_short.rs:83-140), the bits are not.
 * PHILOX_FULL: PHILOX, and the draws of the PLAN from Philox counters as well — what north_star describes ("random
 *   start-position draw, length draw, per-base draws: counter-based"), and what makes a shard's plan a function of its
 *   pair indices alone (no stream to walk or to seek in: the plan path costs a quarter).  Specification, version 1:
 *     every generator the reference seeds on the way to a read — StdRng::seed_from_u64(s) for the lengths
 *     (minimal_short.rs:33-67), the start position and the two mate-2 seeds (simulate.rs:227-270), a long read's own
 *     generator — is the word stream W(s): word w = word w & 3 of the Philox4x32-10 block with key = s and counter
 *     (w >> 2, 3, 0x73696D6D, 0x72000003), consumed in the reference's order by the reference's algorithms (gen_range with
 *     its rejection zone, the ziggurat, Gamma, Option<u64>);
 *     the genome's outer stream (simulate.rs:172-186, one generator walked pair by pair) becomes one block per pair: pair p
 *     of the genome's run (p < 2^56) takes the block with key = the run's seed and counter (p & 0xffffffff, 4 | (p >> 32) << 8,
 *     0x73696D6D, 0x72000003) = (w0, w1, w2, w3): contig = ((w0 | w1 << 32) * num_seqs) >> 64, pe_seed = w2 | w3 << 32
 *     (as in the reference, every genome of a run sees the same seed);
 *     the per-base draws are PHILOX's, keyed by the seeds this plan makes.
 *   Minimal-short, and minimal-long / perfect-long with SIMMR_LEN_PER_READ (the one constant length of a seeded reference
 *   run, simulate.rs:358, is a property of its stream); not the custom profiles.  Restated in oracle/ (rand08.c: the
 *   generator's second word source; simulate.c: orc_pe_outer_ctr), compared bit for bit; law tests in
 *   tests/test_gpu_parity.py::test_philox_full_*.
 * The second counter word names the domain of a draw: 0 and 1 the two levels of the per-base draws, 2 the k-mer splice,
 * 3 the word streams of the plan, 4 the outer stream — and 5 the strain sites, which belong to a staged genome and to no
 * rng mode: "strain sites, version 1" is stated with simmr_strain_plan below. */
enum simmr_rng_mode { SIMMR_RNG_REFERENCE = 0, SIMMR_RNG_PHILOX = 1, SIMMR_RNG_PHILOX_FULL = 2 };

/* Long-read length policy (Appendix A Q5 of SURVEY.md).
 * REFERENCE: with a seed, get_random_read_length(seed) (simulate.rs:358) is
 *   the same value for every read of the run; reproduced exactly.
 * PER_READ: every read draws its own Gamma length, contig and read seed from
 *   a private StdRng keyed by mix(seed, read index).  This is what the
 *   reference does without --seed (fresh entropy per call), made reproducible.
 *   Selected automatically when has_seed == 0. */
enum simmr_length_mode { SIMMR_LEN_REFERENCE = 0, SIMMR_LEN_PER_READ = 1 };

/* Where a long read starts on its sequence (Appendix A Q6 of SURVEY.md).
 * REFERENCE: simulate.rs:484 draws read_start in [0, read_length) — not in
 *   [0, size - read_length) — so every long read starts within the first
 *   read_length bases of its sequence; reproduced exactly.
 * UNIFORM: read_start = gen_range(0..size - read_length) from the same
 *   StdRng(read_seed), read_end = read_start + read_length (no re-draw is needed):
 *   what simulate_long_read evidently means to do.  An extension; off by default. */
enum simmr_long_start_mode { SIMMR_START_REFERENCE = 0, SIMMR_START_UNIFORM = 1 };

/* Flattened ErrorProfile (trait: error_profiles/base.rs:6-32; construction:
 * cli.rs:229-301).  Plain data, copied by the callee. */
typedef struct simmr_error_profile {
  uint32_t kind;        /* enum simmr_profile_kind                           */
  uint32_t rng_mode;    /* enum simmr_rng_mode                               */
  uint32_t length_mode; /* enum simmr_length_mode (long reads only)          */
  uint16_t read_length; /* --read-length   (cli.rs:126)                      */
  uint16_t insert_size; /* --insert-size   (cli.rs:143)                      */
  uint8_t mean_phred;   /* --mean-phred-score (cli.rs:152)                   */
  uint8_t long_start_mode; /* enum simmr_long_start_mode (long reads only) */
  uint8_t reserved0[2];
  double read_length_std; /* minimal-short: 15.0 (cli.rs:240)               */
  double insert_size_std; /* minimal-short: 75.0 (cli.rs:239)               */
  float gamma_shape;      /* (mean/std)^2, minimal_long.rs:68                */
  float gamma_scale;      /* std^2/mean,   minimal_long.rs:69                */
  const void* custom_model;    /* bincode ErrorModelParams (shared/encoding.rs:102-117) */
  uint64_t custom_model_bytes;
} simmr_error_profile;

/* Contiguous range of global unit indices (pairs for PE, reads for long) that
 * this engine / GPU generates.  Replaces nothing in the reference (it has no
 * sharding); ids stay identical to the single-process run. */
typedef struct simmr_range {
  uint64_t first;
  uint64_t count;
} simmr_range;

/* Result of a plan step: what the emit step will write. */
typedef struct simmr_plan_info {
  uint64_t n_units;      /* pairs (PE) or reads (long) planned in this shard  */
  uint64_t n_reads;      /* 2*n_units for PE, n_units for long                */
  uint64_t total_bases;  /* bytes needed in seq[] and in qual[]               */
  uint64_t seed_used;    /* the seed (given, or drawn from OS entropy)        */
  uint64_t outer_slots;  /* u64 draws consumed from the outer StdRng stream (0 with SIMMR_RNG_PHILOX_FULL: there is none) */
  uint32_t const_read_length; /* long/REFERENCE: the run-wide length, else 0  */
  uint32_t slot_bytes;   /* 0: compact streams; 16: SIMMR_SLOT16 (simmr_engine_set_read_slots) */
} simmr_plan_info;

/* flags[] bits */
#define SIMMR_FLAG_REVCOMP 0x01u     /* ReadMetadata.is_reverse_complement    */
#define SIMMR_FLAG_QSEED_SUBST 0x02u /* mate-2 Phred seed drew None (simulate.rs:266):
                                        the reference uses OS entropy there; we
                                        substitute simmr_entropy_substitute() */
#define SIMMR_FLAG_MSEED_SUBST 0x04u /* same for the mutation seed (simulate.rs:270) */
#define SIMMR_FLAG_REDRAWN 0x08u     /* mate-2 window was re-drawn (simulate.rs:241-247) */

/* SoA replacement of Vec<SimulatedRead> (simulate.rs:27-75).  All pointers are
 * DEVICE pointers owned by the caller.  Read r of a PE shard is mate (r & 1)
 * of pair (r >> 1); mates are interleaved exactly as fastq.rs:32-121 writes
 * them.  Any pointer except seq/qual/seq_off may be NULL to skip that column. */
typedef struct simmr_reads_out {
  uint8_t* seq;       /* ASCII bases, total_bases bytes (no slack needed: every emit kernel bounds its last store;
                         tests/test_gpu_shapes.py runs each of them between canaries at exactly this size) */
  uint8_t* qual;      /* Phred + qual_offset, total_bases bytes               */
  uint64_t* seq_off;  /* n_reads + 1 CSR offsets into seq / qual              */
  uint64_t* start;    /* ReadMetadata.start_pos (mate 2: the larger bound)    */
  uint64_t* end;      /* ReadMetadata.end_pos                                 */
  uint32_t* contig;   /* index of the source Seq inside its genome            */
  uint32_t* genome;   /* staged genome index (long reads span genomes)        */
  uint32_t* read_id;  /* SimulatedRead.id (simulate.rs:85-89), shared by mates */
  uint8_t* flags;     /* SIMMR_FLAG_*                                         */
  uint64_t seq_capacity;   /* bytes available in seq and in qual              */
  uint64_t reads_capacity; /* entries available in the per-read columns       */
  uint32_t qual_offset;    /* 0: raw Phred as SingleRead.quality; 33: FASTQ   */
  uint32_t slot_bytes;     /* the layout the caller expects: 0 (or 1) compact, 16 SIMMR_SLOT16; an emit call whose
                              plan was made for the other layout answers SIMMR_EINVAL                        */
} simmr_reads_out;

/* Layout of seq[] / qual[] (the reference's SingleRead is a heap Vec per read, simulate.rs:27-40: neither layout
 * below is "the" reference layout).
 * compact (default): read r's bases are seq[seq_off[r] .. seq_off[r+1]) and its qualities the same bytes of qual[]:
 *   two byte streams without gaps.
 * SIMMR_SLOT16 (simmr_engine_set_read_slots(e, 16) before the plan call; what INTEGRATION.md's call sequence, the Python
 *   host and simmr-hip select): every read owns a slot of ceil(L / 16) * 16 bytes that starts on a 16-byte boundary of
 *   both streams (total_bases counts the slots), so that the counter-mode emit kernel writes nothing but whole aligned
 *   16-byte groups — no byte-granular stores at the reads' ends.  Qualities are left-aligned in the slot.
 *   Bases are left-aligned too, except for a reverse-complemented mate (SIMMR_FLAG_REVCOMP), whose bases are written
 *   back to front and therefore RIGHT-aligned: its 16-base draw groups then land on aligned 16 bytes as well.
 *     seq_off[r]         = first base of read r in seq[]   (for a reverse-complemented mate not a multiple of 16)
 *     seq_off[r] & ~15   = first quality of read r in qual[]
 *     L(r)               = |end[r] - start[r]|   (seq_off[r+1] - seq_off[r] is NOT the length in this layout)
 *     seq_off[n_reads]   = total_bases
 *   Padding bytes are written as 0 in both streams.  The setting is a preference: the kernels that gain from slots write
 *   them — SIMMR_RNG_PHILOX with the minimal-short, minimal-long and perfect-long profiles — and a plan for any other
 *   profile is made for the compact layout.  simmr_plan_info.slot_bytes says which one a plan got; size the buffers
 *   from total_bases of the same info and pass that slot_bytes on in simmr_reads_out.  simmr_fastq_plan /
 *   simmr_fastq_emit read either layout. */
#define SIMMR_SLOT16 16u

/* Device-side counters a run accumulates (reduced across GPUs by the caller
 * with one all-reduce).  Indices into the uint64 array. */
enum simmr_counter {
  SIMMR_CNT_READS = 0,
  SIMMR_CNT_BASES = 1,
  SIMMR_CNT_ACGT_BASES = 2,
  SIMMR_CNT_SUBSTITUTIONS = 3,
  SIMMR_CNT_OUTER_REJECTS = 4,
  SIMMR_CNT_REDRAWN = 5,
  SIMMR_CNT_SEED_SUBST = 6,
  SIMMR_CNT_QUAL_SUM = 7,
  SIMMR_N_COUNTERS = 8
};

typedef struct simmr_engine simmr_engine; /* opaque */

/* ---- lifetime ---------------------------------------------------------- */
int simmr_abi_version(void);
/* Binds to HIP device `device_ordinal`; fails with SIMMR_ENODEV if there is
 * none or it is not gfx950. */
int simmr_engine_create(int device_ordinal, simmr_engine** out);
void simmr_engine_destroy(simmr_engine* e);
/* Last error text of this engine (or of engine creation when e == NULL). */
const char* simmr_last_error(const simmr_engine* e);
/* All work is enqueued on this hipStream_t (default: the null stream). */
int simmr_engine_set_stream(simmr_engine* e, void* hip_stream);
/* Layout of the reads that plans made FROM NOW ON will emit: 0 (or 1) = compact, SIMMR_SLOT16 = 16-byte read slots
 * wherever the plan's emit kernel writes them (see simmr_reads_out; simmr_plan_info.slot_bytes reports what a plan
 * got).  Anything else: SIMMR_EINVAL.  The plan in force keeps the layout it was made with. */
int simmr_engine_set_read_slots(simmr_engine* e, uint32_t slot_bytes);

/* The plan of the next shard beside the emit of this one.  A run that is generated shard by shard (the reference keeps a
 * whole run in RAM, main.rs:180-206; here `for range: plan, emit, drain`) calls plan k + 1 while the emit of shard k is
 * still on the device; with on != 0 the plan calls run on a stream of the engine's own and write a second set of the
 * buffers an emit reads, so the two overlap — the plan kernels are bound by latency, the emit kernels by instruction
 * issue — instead of queueing behind one another.  The caller's stream (simmr_engine_set_stream) is made to wait for the
 * plan before the call returns, so everything the caller enqueues afterwards sees it: no call sequence changes.  Costs a
 * second set of plan columns (25 bytes per pair / long read).  Off by default; switching synchronises the device. */
int simmr_engine_set_plan_overlap(simmr_engine* e, int on);

/* ---- reference staging -------------------------------------------------- */
/* Replaces the in-RAM `Genome { sequence: Vec<Seq> }` (genome.rs:17-41): the
 * normalised ASCII contigs are packed once into HBM as a flat 2-bit array
 * (A0 C1 G2 T3; base i in bits 2(i mod 16) of word i/16 — the code points of
 * shared/src/encoding.rs:146-152) plus a 1-bit exception plane for 'N' / '-'.
 * contig_len[i] = bytes in contig_ascii[i] (Seq.seq.len()),
 * contig_size[i] = Seq.size (differs only under --contiguous, genome.rs:127);
 * NULL means size == len.
 * A contig may have no bases (contig_len[i] == 0): it is staged and keeps its index, and it shares its
 * first base in the plane and its first position in depth[] with the contig behind it, which owns both.
 * simmr_depth_summarize gives it a row of zeros and no windows, no region (simmr_regions_*) and no site
 * (simmr_strain_*) is ever on it, and of the reads simmr_depth_add is given only one of length 0 at its
 * offset 0 stays inside it (tests/test_gpu_layout_seams.py). */
int simmr_stage_genome(simmr_engine* e, uint32_t genome_idx, uint32_t n_contigs,
                       const uint8_t* const* contig_ascii, const uint64_t* contig_len,
                       const uint64_t* contig_size);
/* Genome::from_fasta's sequence handling on the device (genome.rs:93-137): the
 * host splits the file into records (header lines, body ranges); the device
 * applies needletail's normalize(false) (genome.rs:114: whitespace and line ends
 * dropped, acgt -> ACGT, u/U -> T, . ~ -> -, A C G T N - kept, everything else ->
 * N) and packs in the same pass, so no normalised copy is ever built on the host.
 * body[c] / body_len[c]: the raw bytes between record c's header line and the
 * next header (HOST memory).  base_count[c] receives the record's number of bases.
 * contiguous == 0: records with more than min_size bases become the genome's
 *   sequences, in order (the size filter of main.rs:117-162; pass 0 to keep all);
 *   *n_staged = how many.  With none left the slot is left unstaged.
 * contiguous != 0: one sequence, every record followed by an 'N' (genome.rs:
 *   121-137); its Seq.size counts the bases without the separators. */
int simmr_stage_fasta(simmr_engine* e, uint32_t genome_idx, uint32_t n_records,
                      const uint8_t* const* body, const uint64_t* body_len, int contiguous,
                      uint64_t min_size, uint64_t* base_count, uint32_t* n_staged);
/* Synthetic genome generated on the device: word k of the packed array (32
 * bases) is SplitMix64 output k of `splitmix_seed` (BASELINE.md / SURVEY §8d). */
int simmr_stage_synthetic(simmr_engine* e, uint32_t genome_idx, uint32_t n_contigs,
                          const uint64_t* contig_len, uint64_t splitmix_seed);
/* Copies staged bases back as ASCII (debug / tests). dst is a HOST pointer. */
int simmr_unstage_contig(simmr_engine* e, uint32_t genome_idx, uint32_t contig, uint64_t first,
                         uint64_t count, uint8_t* dst_host);
int simmr_genome_info(const simmr_engine* e, uint32_t genome_idx, uint32_t* n_contigs,
                      uint64_t* total_size);

/* ---- paired-end path ----------------------------------------------------- */
/* simulate_pe_reads_from_genome (simulate.rs:165-190) for one genome:
 * `genome_reads` is the reference's num_reads (mates; num_reads/2 pairs,
 * simulate.rs:179).  Plans pairs [shard.first, shard.first+shard.count) of
 * that genome: outer StdRng stream (contig draw + pe_seed), then per pair read
 * length / insert size / window (simulate_pe_read, simulate.rs:205-258).
 * shard.count == UINT64_MAX means "to the end". */
int simmr_pe_plan(simmr_engine* e, uint32_t genome_idx, const simmr_error_profile* profile,
                  uint64_t genome_reads, int has_seed, uint64_t seed, simmr_range shard,
                  simmr_plan_info* info);
/* Seeking in a genome's outer stream, so that N GPUs sharing one run do not each
 * re-walk the stream from slot 0 to their shard (simulate.rs:172-184 draws, per
 * pair, a contig index by rejection sampling and then pe_seed: the slot where
 * pair p starts depends on every earlier rejection).  The loop is a two-state
 * machine over u64 slots (0: about to draw a contig index, 1: about to draw
 * pe_seed); simmr_outer_summarize walks slots [slot_first, slot_first +
 * slot_count) (both multiples of 8) once and returns, for either state at
 * slot_first, how many pairs complete inside the range and the state after it.
 * Ranks summarize disjoint ranges, exchange the 4 numbers (the path's only other
 * collective, 32 bytes per rank) and compose them; simmr_pe_plan_at then starts
 * at a known position: pair `start_unit` begins at slot `start_slot`
 * (start_unit <= shard.first; start_slot = start_unit = 0 is simmr_pe_plan).  With SIMMR_RNG_PHILOX_FULL there is no stream:
 * the two positions are ignored and the call is simmr_pe_plan. */
typedef struct simmr_outer_summary {
  uint64_t units[2];      /* pairs completed in the range, by state at slot_first */
  uint32_t end_state[2];  /* state after the range */
} simmr_outer_summary;
int simmr_outer_summarize(simmr_engine* e, uint32_t genome_idx, uint64_t seed, uint64_t slot_first,
                          uint64_t slot_count, simmr_outer_summary* out);
int simmr_pe_plan_at(simmr_engine* e, uint32_t genome_idx, const simmr_error_profile* profile,
                     uint64_t genome_reads, uint64_t seed, simmr_range shard, uint64_t start_slot,
                     uint64_t start_unit, simmr_plan_info* info);
/* simulate_pe_reads (simulate.rs:110-150) over several genomes in ONE plan.  The
 * reference loops over the genomes and re-creates the outer StdRng with the same
 * seed for each (simulate.rs:137,172), so genomes with the same number of
 * sequences draw the same (contig, pe_seed) list: it is generated once per
 * distinct count and shared.  genome_reads[g] are the per-genome read counts of
 * the abundance profile; shard is a range of the global pair index (genomes
 * concatenated in the given order — the order in which the reference's global id
 * counter, simulate.rs:85-89, numbers the pairs).  simmr_pe_emit then emits the
 * shard with read_id_base = 0 and fills the `genome` column per read.
 * SIMMR_ENOTSUP for custom profiles (plan those one genome at a time). */
int simmr_pe_plan_multi(simmr_engine* e, uint32_t n_genomes, const uint32_t* genome_idx,
                        const uint64_t* genome_reads, const simmr_error_profile* profile, int has_seed,
                        uint64_t seed, simmr_range shard, simmr_plan_info* info);
/* Emits the planned pairs: bases, qualities, mutations, reverse complement,
 * metadata (simulate.rs:260-299).  read_id_base = id of pair 0 of this genome
 * (the reference's global AtomicU32, simulate.rs:85-89). */
int simmr_pe_emit(simmr_engine* e, uint32_t read_id_base, const simmr_reads_out* out);

/* ---- long-read path ------------------------------------------------------ */
/* simulate_long_reads (simulate.rs:323-406) over all genomes at once (ONE
 * StdRng stream spans every genome, simulate.rs:348-351).  genome_reads[g] is
 * the per-genome read count from the abundance profile.  shard is a range of
 * global read indices (generation order across genomes).
 * Profiles: minimal-long, perfect-long, or SIMMR_CUSTOM with a model whose
 * is_long flag is set (custom_short.rs:540-542): then the run-wide length is
 * floor(Normal(read_length_mean, read_length_std)) (custom_short.rs:286-301),
 * qualities come from the per-position PDFs (:332-353) and simmr_long_emit
 * applies simulate_errors, the k-mer splice (:455-516); with
 * SIMMR_LEN_PER_READ every read draws its own length from that Normal law.
 * A custom model needs kmer_size <= 10 (else SIMMR_ENOTSUP); an alternate
 * k-mer that deletes bases makes the reference panic and simmr_long_emit
 * return SIMMR_ERANGE.  custom_model is read during the plan call only; the
 * engine keeps the device tables of the last model it was given (keyed by the
 * model's bytes), so planning many shards with one model builds them once. */
int simmr_long_plan(simmr_engine* e, uint32_t n_genomes, const uint32_t* genome_idx,
                    const uint64_t* genome_reads, const simmr_error_profile* profile, int has_seed,
                    uint64_t seed, simmr_range shard, simmr_plan_info* info);
int simmr_long_emit(simmr_engine* e, uint32_t read_id_base, const simmr_reads_out* out);

/* ---- counters across GPUs ---------------------------------------------------
 * The path has one exchange step: the sum of the run counters over the GPUs of a
 * run.  One engine per process and device; rank 0 makes an id and hands it to the other ranks by
 * whatever channel the host has; every rank then joins.  RCCL is loaded at run time
 * (librccl.so.1), so a single-GPU user needs none.  Replaces nothing in the reference (it is a
 * single process); the counters are what a maintainer would log next to the metadata TSV. */
#define SIMMR_COMM_ID_BYTES 128
int simmr_comm_unique_id(uint8_t* id128);                                   /* ncclGetUniqueId */
int simmr_comm_init(simmr_engine* e, const uint8_t* id128, int rank, int world);  /* ncclCommInitRank on the engine's device */
/* In-place sum over the ranks of n u64 values in device memory (ncclAllReduce on the engine's
 * stream; asynchronous like the rest).  Without a communicator (one GPU) it does nothing. */
int simmr_allreduce_counts(simmr_engine* e, uint64_t* counts_device, uint32_t n);

/* ---- counters / timing ---------------------------------------------------- */
/* Copies the SIMMR_N_COUNTERS running counters to a DEVICE array (for the
 * caller's all-reduce) and/or a HOST array; either may be NULL.  The device
 * copy is enqueued on the engine's stream like everything else (a collective
 * launched from another stream has to be ordered after it by the caller; with
 * the default null stream, as torch.distributed uses it, that is implicit);
 * the host copy is complete on return. */
int simmr_counters(simmr_engine* e, uint64_t* dst_device, uint64_t* dst_host);
int simmr_counters_reset(simmr_engine* e);
/* HIP-event time (ms) of the dominant emit kernel of the last *_emit call,
 * measured on the engine's stream. Synchronises the stream. */
int simmr_last_emit_kernel_ms(simmr_engine* e, float* ms);
/* The mean of the last `last_n` emits' times (at most 64 are kept), after ONE synchronisation of the engine's stream —
 * for a loop that must not wait for every emit (simmr_engine_set_plan_overlap: asking after each emit would serialise
 * the plan of the next shard behind it). */
int simmr_emit_kernel_ms_mean(simmr_engine* e, uint32_t last_n, float* ms);
/* HIP-event time (ms) of the last *_plan call's device work. */
int simmr_last_plan_ms(simmr_engine* e, float* ms);

/* ---- documented substitutions --------------------------------------------- */
/* Where the reference re-seeds from OS entropy in the middle of a seeded run
 * (Option<u64>::None at simulate.rs:266,270) we substitute this pure function
 * of (pe_seed, which) so the run stays reproducible; which = 1 for the Phred
 * seed, 2 for the mutation seed.  Also used to derive per-read seeds in
 * SIMMR_LEN_PER_READ mode (which = 3, x = seed ^ read index mix). */
uint64_t simmr_entropy_substitute(uint64_t x, uint32_t which);

/* ---- FASTQ framing on the device: replaces fastq::write_to_fastq
 * (simmr/src/fastq.rs:14-124) up to the file write.  The record of read r is
 *     header '\n' bases '\n' '+' '\n' qualities '\n'      (fastq.rs:58-66, 93-103)
 * with the header built from `header_format` by the reference's chain of
 * String::replace calls (fastq.rs:34-56, 69-91): {:genome_id:} {:read_id:}
 * {:sequence_id:} {:start_position:} {:end_position:} {:reverse_complement:}
 * (t / f) {:pair:} (1 / 2).  Qualities are copied as they are: emit them with
 * qual_offset = 33 (util::encode_quality_scores, util.rs:46-57).
 *
 * names: the text of {:genome_id:} per genome (Genome.uuid, main.rs:73-75) and of
 * {:sequence_id:} per contig (Seq.id, genome.rs:100-112), for every engine genome
 * slot the reads' `genome` column can hold.
 *
 * simmr_fastq_plan sizes every record (device), scans the sizes and returns the
 * total; simmr_fastq_emit writes the n_reads records back to back into dst
 * (device memory, >= total bytes).  `reads` must carry every column.
 *
 * SIMMR_ENOTSUP (nothing written; use the host writer): a genome or sequence id
 * containing '{' or '}' (the chained replace could then re-expand it), a template
 * whose own text has a '{' somewhere before and a '}' somewhere after a
 * {:genome_id:} or {:sequence_id:} field (the inserted id could complete a
 * placeholder with them), more than 24 template pieces, or a header longer than
 * 255 bytes.  SIMMR_EINVAL: a genome_idx entry that is not a staged slot. */
typedef struct simmr_fastq_names {
  uint32_t n_genomes;
  const uint32_t* genome_idx;      /* engine genome slot of each entry */
  const char* const* genome_id;    /* NUL-terminated */
  const uint32_t* n_contigs;       /* contigs of each entry, as staged */
  const char* const* sequence_id;  /* flattened entry by entry, NUL-terminated */
} simmr_fastq_names;

int simmr_fastq_plan(simmr_engine* e, const char* header_format, const simmr_fastq_names* names,
                     const simmr_reads_out* reads, uint64_t n_reads, int paired, uint64_t* total_bytes);
int simmr_fastq_emit(simmr_engine* e, const simmr_reads_out* reads, uint8_t* dst, uint64_t dst_capacity);

/* The same text without the columns in between: what main.rs:180-206 does as a whole — simulate, then
 * fastq::write_to_fastq (fastq.rs:14-124) — for the shard of the CURRENT plan (simmr_pe_plan / simmr_pe_plan_at /
 * simmr_pe_plan_multi / simmr_long_plan).  A header's length depends on plan columns only (decimal widths of read id,
 * start and end; the lengths of the ids), so
 *   simmr_fastq_plan_direct sizes every record from the plan and returns the total, and
 *   simmr_emit_fastq writes the shard's records back to back into dst (device memory, >= total bytes): the emit kernel
 *     stores bases and qualities (offset 33, util.rs:46-57) at their places in the text and formats the headers and
 *     line ends of its block's records itself.  The run counters advance as simmr_*_emit advances them (for a
 *     perfect-short run on a genome with N / '-' bases SIMMR_CNT_ACGT_BASES is counted here, which simmr_pe_emit
 *     leaves at 0).
 * The bytes are those of simmr_*_emit (qual_offset 33) + simmr_fastq_plan + simmr_fastq_emit with the same arguments,
 * and the same cases are refused with SIMMR_ENOTSUP.  Served by a kernel that writes into the text: the counter mode
 * (SIMMR_RNG_PHILOX) of the minimal / perfect-long profiles, and perfect-short (no draws: the planned bases and a
 * constant quality line).  Profiles whose emit kernel cannot write into text (SIMMR_RNG_REFERENCE, custom models) are
 * served through columns held by the engine: same result, no saving. */
int simmr_fastq_plan_direct(simmr_engine* e, const char* header_format, const simmr_fastq_names* names,
                            uint32_t read_id_base, uint64_t* total_bytes);
int simmr_emit_fastq(simmr_engine* e, uint8_t* dst, uint64_t dst_capacity);
/* HIP-event time (ms) of the last simmr_fastq_plan_direct's device work (size pass + scan). */
int simmr_last_fastq_plan_ms(simmr_engine* e, float* ms);

/* ---- ground truth per read: which bases of a read are not the reference's -------------------------------------
 * Replaces nothing in the reference (it records where a read came from, never what it changed); it is what a caller
 * who scores an aligner, an error corrector or a variant caller needs next to the reads.
 *
 * What counts as an edit.  For read r, L = |end[r] - start[r]| and lo = min(start[r], end[r]); the coordinates index
 * Seq.seq of contig contig[r] of genome slot genome[r], as simmr_unstage_contig sees them.  The EXPECTED byte at offset
 * j (0 <= j < L) of the read as written is
 *   the staged base at lo + j                            for a forward read,
 *   complement(staged base at lo + L - 1 - j)            for a read with SIMMR_FLAG_REVCOMP (util.rs:15-37);
 * a staged 'N' or '-' is expected as itself (the exception plane) and is its own complement.  An EDIT is an offset whose
 * byte in seq[] differs from the expected byte.  The edits of a read come in ascending edit_pos, reads in order, so
 * nm[r] = edit_off[r + 1] - edit_off[r].  No profile of a successful run changes a read's length (a deleting splice
 * already answers SIMMR_ERANGE), so every edit is a substitution: insertions and deletions are out of scope.
 *
 * The pass is a diff of seq[] as the caller hands it over against the staged planes, not a replay of the draws: it
 * serves every profile, every rng mode, both layouts (reads->slot_bytes 0 and SIMMR_SLOT16, with the right-aligned
 * reverse mates), paired and long reads, columns of any plan call — and bytes changed after the emit.  The result is a
 * function of the inputs alone: edits are counted, the counts scanned, then written at their ranks (no atomics hand out
 * slots), so launch geometry never changes a byte.
 *
 * `reads` must carry seq, qual, seq_off, start, end, contig, genome and flags (read_id may be NULL), with seq_capacity
 * >= seq_off[n_reads] as for the emit that filled them. */
typedef struct simmr_truth_out {       /* DEVICE pointers, caller-owned */
  uint32_t* nm;         /* n_reads: altered bases of read r                                  */
  uint64_t* edit_off;   /* n_reads + 1: CSR offsets into the edit columns                    */
  uint32_t* edit_pos;   /* 0-based offset in the read AS WRITTEN (read orientation)          */
  uint8_t*  edit_ref;   /* ASCII base the unaltered read would carry there                   */
  uint8_t*  edit_alt;   /* ASCII base the read carries                                       */
  uint8_t*  edit_qual;  /* the byte of qual[] at that position, as stored (qual_offset kept) */
  uint64_t  reads_capacity, edits_capacity;
} simmr_truth_out;
/* Counts the edits of every read and scans the counts into buffers the engine holds; *n_edits = their total.
 * SIMMR_EINVAL: a missing required column, or a read whose genome / contig entry is not staged or whose coordinates
 * leave its contig or seq[] (found by a bounds check on the device and reported through an error word: such a read is
 * never loaded from). */
int simmr_truth_plan(simmr_engine* e, const simmr_reads_out* reads, uint64_t n_reads, uint64_t* n_edits);
/* Writes the columns for the SAME reads.  nm and any edit_* may be NULL to skip that column; edit_off is required when
 * an edit_* column is given.  SIMMR_ESTATE: no simmr_truth_plan for these columns (same seq, seq_off and layout).
 * SIMMR_ERANGE, nothing written: reads_capacity < n_reads (with nm or edit_off given) or edits_capacity < n_edits (with
 * an edit_* column given).
 * Between the plan and the emit seq[], the columns and the staged genomes must stay as they were: the emit finds the
 * edits again and places them by the plan's offsets.  Staging a genome discards the plan (SIMMR_ESTATE); bytes of seq[]
 * changed in between are not detected — no store leaves a read's own range of the edit columns, but entries of that
 * range may then be left unwritten or hold the changed bytes' edits. */
int simmr_truth_emit(simmr_engine* e, const simmr_reads_out* reads, const simmr_truth_out* out);
/* HIP-event time (ms) of the last simmr_truth_plan's device work (count + scan) plus that of the simmr_truth_emit after
 * it, if any.  Synchronises the stream. */
int simmr_last_truth_ms(simmr_engine* e, float* ms);

/* ---- run statistics: quality, base and mismatch tables of the reads of a run ------------------------------------
 * Replaces nothing in the reference.  The eight run counters are sums; these tables are the distributions a user of a
 * read simulator looks at — quality per cycle, base composition, which substitutions occurred, how often a base of
 * Phred q was altered — counted on the device from the columns in HBM, without draining the reads.
 *
 * Definitions.  EXPECTED byte, EDIT, lo and L = |end[r] - start[r]| are exactly simmr_truth_out's (above): coordinates
 * into Seq.seq, reverse mates complemented, a staged 'N' or '-' expected as itself.  The WRITTEN byte at offset j is
 * seq[seq_off[r] + j]; the quality at offset j is qual[qbase + j] with qbase = seq_off[r] (compact) or seq_off[r] & ~15
 * (SIMMR_SLOT16), and q = (that byte - reads->qual_offset) & 255.  A byte's CLASS is 0 1 2 3 for 'A' 'C' 'G' 'T' and 4
 * ("other") for every other byte, 'N' and '-' among them.  Read r belongs to SET r % n_sets: n_sets = 2 for a paired
 * shard (mate 1 / mate 2), 1 for long reads (everything in set 0).
 * Offsets at or above SIMMR_STATS_CYCLES enter every table except the four cycle_* ones (they are not clamped into a
 * last bin).
 *
 * Every table is an integer sum over reads, so the result is a function of the inputs alone — launch geometry never
 * changes a number — and the tables of several adds, ranges, engines or ranks add up entry by entry (the caller sums
 * them; the library offers no all-reduce for them). */
#define SIMMR_STATS_CYCLES  512u   /* per-cycle tables cover offsets 0..511 of a read as written */
#define SIMMR_STATS_NM_BINS 64u

typedef struct simmr_run_stats {            /* HOST memory, every entry a uint64_t */
  uint64_t reads[2];                        /* reads of set m, L = 0 included */
  uint64_t bases[2];                        /* sum of L */
  uint64_t qual_n[256];                     /* bases by q = (qual byte - qual_offset) & 255 */
  uint64_t qual_mismatch[256];              /* of those, edits (simmr_truth_out's definition of an edit) */
  uint64_t pair[5][5];                      /* [expected class][written class], classes A C G T other; every base counted once */
  uint64_t nm_hist[SIMMR_STATS_NM_BINS];    /* reads (L = 0 included) by number of edits, clamped to the last bin */
  uint64_t gc_hist[101];                    /* reads with L > 0 by floor(100 * (#'G' + #'C' written) / L) */
  uint64_t cycle_n[2][SIMMR_STATS_CYCLES];  /* reads of set m with L > j */
  uint64_t cycle_qsum[2][SIMMR_STATS_CYCLES];      /* sum of q at offset j */
  uint64_t cycle_mismatch[2][SIMMR_STATS_CYCLES];  /* edits at offset j */
  uint64_t cycle_base[2][SIMMR_STATS_CYCLES][5];   /* written class at offset j */
} simmr_run_stats;

/* Allocates the engine's tables on first use and zeroes them and the sticky error (on the engine's stream). */
int simmr_stats_reset(simmr_engine* e);
/* Adds the reads of `reads` to the tables.  Only enqueues on the engine's stream — no synchronisation — so it can sit in
 * a step loop beside the emit; staging a genome afterwards does not discard the tables (they are sums over reads already
 * seen), but the genomes the columns name must be staged when the add runs.
 * `reads` must carry seq, qual, seq_off, start, end, contig, genome and flags (read_id may be NULL).
 * SIMMR_EINVAL, at once: n_sets other than 1 or 2, or a missing required column.  SIMMR_ESTATE: no simmr_stats_reset yet.
 * A read whose genome or contig entry is not staged, whose window leaves its contig or seq[] (simmr_truth_plan's bounds
 * check), or which is longer than 65 535 bases (the longest read the library writes; the bound keeps the kernel's 32-bit
 * partial counts from wrapping) is never loaded from: it sets a sticky error word, simmr_stats_read then answers
 * SIMMR_EINVAL and copies nothing, and the tables are unspecified until the next simmr_stats_reset. */
int simmr_stats_add(simmr_engine* e, const simmr_reads_out* reads, uint64_t n_reads, uint32_t n_sets);
/* Synchronises the stream and copies the tables to *dst_host.  SIMMR_ESTATE before any simmr_stats_reset. */
int simmr_stats_read(simmr_engine* e, simmr_run_stats* dst_host);
/* HIP-event time (ms) of the last simmr_stats_add's device work.  Synchronises the stream. */
int simmr_last_stats_ms(simmr_engine* e, float* ms);

/* ---- coverage depth: where the reads of a run landed, per position, window and contig ----------------------------
 * Replaces nothing in the reference, which reports the nominal num_reads and abundance of a genome (files.rs:100-134) and
 * never what a run put on each contig.  Counted on the device from four columns in HBM, without draining the reads.
 *
 * Definition.  For read r, L = |end[r] - start[r]| and lo = min(start[r], end[r]): coordinates into Seq.seq, exactly
 * simmr_truth_out's (above).  The read COVERS positions lo .. lo + L - 1 of contig contig[r] of genome slot genome[r]; a
 * read with L = 0 covers nothing.  depth[x] = the number of added reads that cover x.  Mates count separately (an
 * overlapping pair contributes 2 where it overlaps): read depth, not fragment depth.
 * depth[] is ONE dense uint32_t array over every genome staged when simmr_depth_reset was called: genomes in ascending slot
 * order, the contigs of a genome in order, each contig Seq.seq.len() entries, no padding; n_positions is the total, and
 * simmr_depth_contig_first says where a contig starts.
 *
 * Every result is an integer sum over reads, so it is a function of the inputs alone — launch geometry and the order of
 * the adds never change a number — and the arrays of several adds, ranges, engines or ranks add up entry by entry (the
 * caller sums them; the library offers no all-reduce for them). */
#define SIMMR_DEPTH_HIST_BINS 256u

typedef struct simmr_depth_contig {   /* HOST memory: one row per tracked contig, in the order of depth[] */
  uint32_t genome, contig;            /* genome slot, contig index */
  uint64_t first, len;                /* the contig is depth[first .. first + len) */
  uint64_t covered;                   /* positions with depth >= 1 */
  uint64_t depth_sum;                 /* sum of depth over the contig = bases of the reads that landed on it */
  uint32_t depth_max, reserved0;
  uint64_t first_window;              /* index of the contig's first window in the window columns (window > 0), else 0 */
} simmr_depth_contig;

typedef struct simmr_depth_windows {  /* DEVICE pointers, caller-owned: one entry per window */
  uint64_t* sum;                      /* sum of depth over the window */
  uint32_t* covered;                  /* positions of the window with depth >= 1 */
  uint32_t* max;
  uint64_t capacity;                  /* entries available in each column */
  uint64_t n_windows;                 /* OUT: windows of the run, written whenever the layout is known (also with
                                         SIMMR_ERANGE, so that a caller can size the columns and call again) */
} simmr_depth_windows;

/* Allocates on first use and zeroes (on the engine's stream) the engine's difference array — n_positions + 1 int32_t —
 * and its sticky error word, and records which genomes are tracked: those staged now.  *n_positions receives the length
 * of depth[], *n_contigs the number of tracked contigs (the rows of simmr_depth_summarize); either may be NULL.
 * SIMMR_ENOMEM if the array cannot be had. */
int simmr_depth_reset(simmr_engine* e, uint64_t* n_positions, uint64_t* n_contigs);
/* Adds the reads of `reads`.  Only enqueues on the engine's stream — no synchronisation.  Needs start, end, contig and
 * genome; seq, qual and seq_off are not read and may be NULL here.
 * SIMMR_ESTATE: no simmr_depth_reset yet, or a genome was staged since (the layout of depth[] is the reset's).
 * SIMMR_ERANGE: the reads added since the reset would reach 2^31 (the bound keeps every int32_t partial from wrapping).
 * A read whose genome slot is not tracked, whose contig does not exist or whose window leaves its contig adds nothing and
 * sets the sticky error word (the check comes before any address is formed from the read). */
int simmr_depth_add(simmr_engine* e, const simmr_reads_out* reads, uint64_t n_reads);
/* Scans the difference array into depth_device (DEVICE memory, 16-byte aligned, `capacity` uint32_t entries) and
 * synchronises.  The difference array is left as it is: adds may go on and a later emit sees all of them.
 * SIMMR_ESTATE: no simmr_depth_reset yet.  SIMMR_ERANGE, nothing written: capacity < n_positions.  SIMMR_EINVAL: the sticky
 * error word is set (depth_device is then unspecified, and stays so until the next simmr_depth_reset). */
int simmr_depth_emit(simmr_engine* e, uint32_t* depth_device, uint64_t capacity);
/* Host arithmetic: *first = where contig `contig` of genome slot `genome_idx` starts in depth[].  SIMMR_ESTATE before a
 * reset, SIMMR_EINVAL for a slot or contig the reset did not track. */
int simmr_depth_contig_first(simmr_engine* e, uint32_t genome_idx, uint32_t contig, uint64_t* first);
/* Summarises a depth[] array of the layout of the last reset (depth_device: n_positions entries in DEVICE memory — what
 * simmr_depth_emit wrote, or a sum of such arrays) and synchronises.
 *   rows_host[k], k < the number of tracked contigs (rows_capacity must hold them, else SIMMR_ERANGE): see the struct;
 *   hist_host[SIMMR_DEPTH_HIST_BINS]: positions by depth, clamped to the last bin; its sum is n_positions;
 *   window > 0 with win != NULL: the three columns per window.  Contig k has ceil(len / window) windows, the last one
 *     partial, at first_window(k) onwards; windows never span contigs.  SIMMR_ERANGE (nothing written) if win->capacity is
 *     smaller than their number, which win->n_windows receives either way.  window must be below 2^30 (SIMMR_EINVAL).
 * rows_host and hist_host may be NULL to skip them.  window == 0 or win == NULL: no window columns. */
int simmr_depth_summarize(simmr_engine* e, const uint32_t* depth_device, uint32_t window, simmr_depth_contig* rows_host,
                          uint64_t rows_capacity, uint64_t* hist_host, simmr_depth_windows* win);
/* HIP-event time (ms) of the last simmr_depth_add's device work plus that of the simmr_depth_emit and the
 * simmr_depth_summarize after it, if any.  Synchronises the stream. */
int simmr_last_depth_ms(simmr_engine* e, float* ms);

/* ---- strain divergence: a genome that is N % identical to the one that was staged --------------------------------
 * Replaces nothing in the reference, whose --with-ani flag ("Generate reads with an average identity of N (compared to
 * their reference)", cli.rs:185-191) is declared and never read.  Average nucleotide identity is a property of a strain:
 * the same differences in every read that covers a site, which no per-read error rate gives.  The pass substitutes bases
 * of a staged genome IN PLACE in its 2-bit plane (no second copy of the genome) and lists the sites.  Substitutions keep
 * every coordinate, so plans, headers, depth and statistics work unchanged on the diverged genome; simmr_truth_* diffs
 * reads against the genome they were drawn from — the diverged one — and so keeps reporting the sequencing errors, while
 * the site list reports the strain's differences: together the full truth against the original assembly.
 *
 * Strain sites, version 1 (restated in DESIGN.md section 4 and, independently, in tests/_strain.py, which the kernels are
 * compared with byte for byte).  Inputs: a staged genome, identity (a double, 0.25 <= identity <= 1), a 64-bit seed.
 *   T32 = floor((1 - identity) * 2^32 + 0.5) (at most 3 * 2^30); A = ceil(T32 / 3), B = ceil(2 T32 / 3), in integers.
 *   The base at position pos (0-based, in Seq.seq coordinates as simmr_unstage_contig sees them) of contig c owns ONE
 *   32-bit word X: word pos & 3 of the Philox4x32-10 block with key = (seed low word, seed high word) and counter
 *   (pos >> 2, 5, c, 0x72000003) — domain 5, the next free one after 0-4 (enum simmr_rng_mode).  A contig of 2^34 bases
 *   or more is refused with SIMMR_ENOTSUP, so pos >> 2 fits the first counter word.
 *   The base is a SITE iff X < T32 and it is not under the exception plane: an 'N' or '-' stays what it is, its word is
 *   not used.  At a site s = 1 + (X >= A) + (X >= B) and the new code is (code + s) & 3 over A0 C1 G2 T3 — the alternate
 *   rule of specification 3 of the per-base draws.
 *   identity == 1 gives T32 == 0: no sites, planes unchanged bit for bit.  Padding bases between contigs, the pad words in
 *   front of and behind the plane and the exception plane are never written.
 * The result is a function of (planes, identity, seed) alone: sites are counted per tile, the counts scanned, the sites
 * written at their ranks (no atomics hand out slots), so launch geometry never changes a byte. */
typedef struct simmr_strain_out {   /* DEVICE pointers, caller-owned; any column may be NULL */
  uint32_t* contig;                 /* index of the site's Seq inside the genome                       */
  uint64_t* pos;                    /* 0-based position in Seq.seq                                     */
  uint8_t* ref;                     /* ASCII base before the apply                                     */
  uint8_t* alt;                     /* ASCII base after it                                             */
  uint64_t capacity;                /* entries available in each column                                */
} simmr_strain_out;
/* Counts the sites per tile and scans the counts into buffers the engine holds; *n_sites = their total.  Changes nothing
 * else.  SIMMR_EINVAL: the slot is not staged, identity is outside [0.25, 1] or NaN.  SIMMR_ENOTSUP: see above. */
int simmr_strain_plan(simmr_engine* e, uint32_t genome_idx, double identity, uint64_t seed, uint64_t* n_sites);
/* Draws again, writes the sites at their ranks — ordered by contig, then by pos ascending — and rewrites the 2-bit plane
 * in place; synchronises.  out may be NULL (or every column NULL): the genome is diverged all the same.
 * Counts as a staging call: the truth plan is dropped and the staging epoch counts on exactly as in simmr_stage_genome,
 * and the plan in force is dropped too (plan again before the next emit).  The strain plan is consumed: a second apply
 * answers SIMMR_ESTATE, so a genome is not diverged twice by accident.
 * SIMMR_ESTATE: no simmr_strain_plan for that genome, or a staging call since.  SIMMR_ERANGE, nothing written, the planes
 * included, and the plan kept: a column is given and capacity < n_sites. */
int simmr_strain_apply(simmr_engine* e, uint32_t genome_idx, const simmr_strain_out* out);
/* HIP-event time (ms) of the last simmr_strain_plan's device work (count + scan) plus that of the simmr_strain_apply after
 * it, if any.  Synchronises the stream. */
int simmr_last_strain_ms(simmr_engine* e, float* ms);

/* ---- gold-standard assembly: the covered regions of every genome and their bases ------------------------------------
 * Replaces nothing in the reference.  The stretches of every genome that a run covered well enough to be assembled, as
 * coordinates and as sequence: what assemblers and binners are scored against.  depth[], the 2-bit planes and the contig
 * tables already sit in HBM; this pass turns them into a region list and a base stream without copying either to the host
 * — and after simmr_strain_apply the planes are the only place where the strain's sequence exists.
 *
 * Inputs.  depth_device: a uint32_t array of n_positions entries in the layout of the last simmr_depth_reset — what
 * simmr_depth_emit wrote, or an entry-wise sum of such arrays; min_depth >= 1; min_len >= 1.
 * Run.  A maximal set of consecutive positions of one contig with depth[x] >= min_depth.  Runs never span contigs:
 * depth[] has no padding between contigs, so a run that reaches a contig's last position ends there even if the next
 * contig's first position qualifies.
 * Region.  A run of at least min_len positions.
 * Order.  Regions are ordered as depth[] is: genome slot, contig, start ascending.
 * Per region k: genome[k], contig[k]; start[k], 0-based, in Seq.seq coordinates as simmr_unstage_contig sees them; len[k];
 * depth_sum[k], the sum of depth[x] over the region, 64-bit; seq_off[k], the exclusive prefix sum of len;
 * seq_off[n_regions] = n_bases.
 * Base stream.  seq[seq_off[k] .. seq_off[k] + len[k]) holds the ASCII bases of the region as staged now: byte for byte
 * what simmr_unstage_contig(genome, contig, start, len) returns — 'N' and '-' as themselves, the strain's bases after
 * simmr_strain_apply.  There are no separators.
 * Determinism.  Every output is a function of (depth[], planes, min_depth, min_len) alone: ranks come from counts and
 * scans, never from an atomic that hands out slots (depth_sum is summed with integer atomic adds, whose order changes
 * nothing). */
typedef struct simmr_regions_out {   /* DEVICE pointers, caller-owned; any column may be NULL */
  uint32_t* genome; uint32_t* contig; uint64_t* start; uint64_t* len; uint64_t* depth_sum;
  uint64_t* seq_off;                 /* n_regions + 1 entries */
  uint64_t capacity;                 /* regions each column holds (seq_off: capacity + 1) */
  uint8_t* seq; uint64_t seq_capacity; /* the base stream, 16-byte aligned, and the bytes it holds; NULL skips the bases */
} simmr_regions_out;
/* Counts the runs per tile, scans, pairs run starts with run ends, flags the regions among the runs and ranks them — all
 * into buffers the engine holds (sized from the counted runs and regions, not from n_positions); writes nothing to the
 * caller's buffers but *n_regions and *n_bases.  Runs on the engine's stream and synchronises.  depth_device is 16-byte
 * aligned.
 * SIMMR_ESTATE: no simmr_depth_reset yet, or a staging call since (the epoch check of simmr_depth_add).  SIMMR_EINVAL:
 * min_depth == 0 or min_len == 0.  SIMMR_ENOMEM: the run buffers cannot be had. */
int simmr_regions_plan(simmr_engine* e, const uint32_t* depth_device, uint32_t min_depth, uint64_t min_len, uint64_t* n_regions,
                       uint64_t* n_bases);
/* Writes the columns that are given and, if out->seq is given, the base stream; synchronises.  The call is made with the
 * SAME depth_device contents as the plan: the regions are the plan's, and depth[] is read again only for depth_sum (over
 * the plan's regions; it may be NULL when depth_sum is).  The plan stays valid for repeated emits until the next
 * simmr_regions_plan, simmr_depth_reset or staging call.
 * SIMMR_ESTATE: no plan for this epoch.  SIMMR_ERANGE, nothing written, the plan kept: a column is given and capacity <
 * n_regions, or seq is given and seq_capacity < n_bases. */
int simmr_regions_emit(simmr_engine* e, const uint32_t* depth_device, const simmr_regions_out* out);
/* HIP-event time (ms) of the last simmr_regions_plan (first launch to last, the two read-backs of counts in between
 * included) plus that of the simmr_regions_emit after it, if any.  Synchronises the stream. */
int simmr_last_regions_ms(simmr_engine* e, float* ms);

/* ---- allele counts at listed sites: what the reads of a run show at every site of a list ---------------------------------
 * Replaces nothing in the reference.  What a variant truth set carries per site next to REF and ALT — depth and allele
 * depth, per strand (DP, AD, ADF, ADR) — counted on the device from the columns in HBM, without draining the reads: a site
 * nobody covered cannot be called, and a site covered three times is not the truth a site covered sixty times is.
 *
 * Site list.  n triples (genome slot, contig, pos) in device memory, strictly ascending by (slot, contig, pos): the order of
 * depth[], and the order in which simmr_strain_apply writes one genome's sites, so the lists of several genomes concatenate
 * in slot order.  pos is 0-based in Seq.seq coordinates as simmr_unstage_contig sees them.
 * Covering.  For read r, L = |end[r] - start[r]| and lo = min(start[r], end[r]), exactly simmr_truth_out's.  The read
 * COVERS a site iff genome[r] and contig[r] are the site's and lo <= pos < lo + L (a read with L = 0 covers nothing).
 * Written byte.  j = pos - lo for a forward read, j = L - 1 - (pos - lo) for a read with SIMMR_FLAG_REVCOMP; the byte is
 * seq[seq_off[r] + j] in both layouts (seq_off[r] is the read's first base in SIMMR_SLOT16 too).  Its CLASS is the
 * statistics pass's: 0 1 2 3 for 'A' 'C' 'G' 'T' and 4 for every other byte.
 * Observed class, in genome orientation: the class itself for a forward read; for a reverse read its complement, 0 <-> 3
 * and 1 <-> 2, while 4 stays 4.
 * counts[s][strand][class] += 1 for every read that covers site s, strand = 1 for a reverse read: the table is
 * uint32_t counts[n][2][5].  Mates count separately, as in read depth — INVARIANT: the ten counts of site s sum to
 * depth[x] of its position for the same reads.
 *
 * Every entry is an integer sum over reads, so the result is a function of the inputs alone — launch geometry and the order
 * of the adds never change a number — and the tables of several adds, ranges or engines add up entry by entry. */
typedef struct simmr_pileup_sites {     /* DEVICE pointers, caller-owned */
  const uint32_t* genome; const uint32_t* contig; const uint64_t* pos; uint64_t n;
} simmr_pileup_sites;
/* Records the dense layout of the genomes staged now (depth[]'s: genomes in ascending slot order, contigs in order, no
 * padding; no simmr_depth_reset is needed), turns every site into a 64-bit key first(slot, contig) + pos in a buffer the
 * engine holds, allocates and zeroes counts and the sticky error word, and synchronises: the caller's columns are not needed
 * after the call.  n == 0 is valid (adds then do nothing).
 * SIMMR_EINVAL, found on the device before a key is used as an address anywhere: a site whose slot is not staged, whose
 * contig does not exist, whose pos is not below the contig's length, or that does not come after the site before it (out of
 * order, or repeated); simmr_last_error names the index of the first such site.  No table is then in force.
 * SIMMR_ENOMEM if the buffers cannot be had. */
int simmr_pileup_reset(simmr_engine* e, const simmr_pileup_sites* sites);
/* Adds the reads of `reads`.  Only enqueues on the engine's stream — no synchronisation.  Needs seq, seq_off, start, end,
 * contig, genome and flags; qual is not read.
 * SIMMR_ESTATE: no simmr_pileup_reset yet, or a genome was staged since (simmr_strain_apply counts as staging: reset after
 * it).  SIMMR_ERANGE: the reads added since the reset would reach 2^31 (the bound keeps a uint32_t count from wrapping).
 * A read whose genome slot is not tracked, whose contig does not exist, whose window leaves its contig or whose bytes would
 * leave seq[0 .. seq_capacity) is never loaded from: it adds nothing and sets the sticky error word (simmr_truth_plan's
 * bounds check, made before any address is formed from the read). */
int simmr_pileup_add(simmr_engine* e, const simmr_reads_out* reads, uint64_t n_reads);
/* Synchronises, then copies the table — n * 10 uint32_t — to counts_device (DEVICE memory holding capacity_sites * 10
 * entries).  The engine's table is left as it is: adds may go on and a later read sees all of them.
 * SIMMR_ESTATE: no simmr_pileup_reset yet.  SIMMR_ERANGE, nothing written: capacity_sites < n.  SIMMR_EINVAL, nothing
 * written: the sticky error word is set (it stays so until the next simmr_pileup_reset). */
int simmr_pileup_read(simmr_engine* e, uint32_t* counts_device, uint64_t capacity_sites);
/* HIP-event time (ms) of the last simmr_pileup_add's device work.  Synchronises the stream. */
int simmr_last_pileup_ms(simmr_engine* e, float* ms);

/* ---- the true alignments as SAM text: one alignment line per read, formatted on the device ---------------------------------
 * Replaces nothing in the reference.  The form of ground truth that samtools, variant callers and aligner-scoring scripts take
 * directly, made from the read columns (simmr_reads_out) and the caller-owned truth columns (simmr_truth_out) that
 * simmr_truth_plan / simmr_truth_emit filled — without draining the reads, and without touching the genome planes: NM and MD
 * need edit_off, edit_pos and edit_ref only.  The lines carry no header: @HD, @SQ and @PG are a few lines for the host.
 *
 * Record of read r.  lo = min(start, end), hi = max(start, end), L = hi - lo, rev = flags & SIMMR_FLAG_REVCOMP.  Eleven
 * tab-separated fields, two tags, '\n':
 *   QNAME  read_id[r] in decimal (mates share it)
 *   FLAG   paired: 0x1 | 0x2 | (rev ? 0x10 : 0) | (rev of read r^1 ? 0x20 : 0) | ((r & 1) ? 0x80 : 0x40); else rev ? 16 : 0
 *   RNAME  the name given for (genome[r], contig[r])
 *   POS    lo + 1
 *   MAPQ   255
 *   CIGAR  <L>M (no profile changes a read's length); for L == 0: *, with SEQ and QUAL * and MD 0
 *   RNEXT PNEXT TLEN   paired: =, lo of read r^1 plus 1, and the signed span; else *, 0, 0.  The span of a pair is max(hi) -
 *          min(lo) over the two mates: positive for the mate with the smaller lo (on a tie mate 1), negative for the other.
 *          Mates of a re-drawn window (SIMMR_FLAG_REDRAWN) follow the same rule.
 *   SEQ    the read on the forward strand: the bytes of seq[] as written, or for a rev read their reverse complement (ACGTN,
 *          other bytes kept); then every byte that is not one of A C G T N is written as N (SAM has no '-')
 *   QUAL   the bytes of qual[] for the read, back to front for a rev read (reads->qual_offset must be 33)
 *   NM:i:  edit_off[r + 1] - edit_off[r]
 *   MD:Z:  forward-strand order: the number of matching bases, a reference base, the next number, and so on; it begins and
 *          ends with a number, so two adjacent edits have 0 between them.  For a rev read the edits are taken from last to
 *          first, at forward offset L - 1 - edit_pos, with edit_ref complemented.  A reference byte outside ACGT is written N.
 * Both layouts are read (for SIMMR_SLOT16 the qualities start at seq_off & ~15 and reverse mates are right-aligned).  `reads`
 * must carry every column, read_id included; `truth` edit_off, edit_pos and edit_ref; with `paired`, n_reads is even.
 *
 * The text is a function of the inputs alone: sizes are counted and scanned, records written at their offsets; no atomic hands
 * out space and launch geometry changes no byte.  No store of record r leaves its own bytes of dst even when the columns were
 * changed between the plan and the emit, and no load leaves a read's own bytes of seq[] / qual[] in either layout. */
typedef struct simmr_sam_names {      /* HOST memory */
  uint32_t n_genomes;
  const uint32_t* genome_idx;         /* engine genome slot of each entry */
  const uint32_t* n_contigs;          /* contigs of each entry, as staged */
  const char* const* rname;           /* RNAME per contig, flattened entry by entry, NUL-terminated */
} simmr_sam_names;
/* Sizes every record on the device, scans the sizes into offsets the engine holds, and returns the total.  Fewer than 2^31
 * reads a call (SIMMR_ERANGE).
 * SIMMR_EINVAL: a required column is missing, qual_offset != 33, `paired` with an odd n_reads, a names entry that is not a staged
 * slot (or not with that many contigs); and, found on the device and reported through an error word, with nothing loaded or
 * stored for that read: a read whose genome / contig has no name, whose seq_off leaves seq_capacity, whose length is above
 * 65 535, whose edit_off decreases or leaves edits_capacity; an edit_pos >= L, or edits that do not ascend within a read.
 * SIMMR_ENOTSUP: an RNAME that is empty, longer than 254 bytes, or outside SAM's
 * [0-9A-Za-z!#$%&+./:;?@^_|~-][0-9A-Za-z!#$%&*+./:;=?@^_|~-]*. */
int simmr_sam_plan(simmr_engine* e, const simmr_sam_names* names, const simmr_reads_out* reads,
                   const simmr_truth_out* truth, uint64_t n_reads, int paired, uint64_t* total_bytes);
/* Writes the n_reads alignment lines back to back into dst (DEVICE memory of at least total_bytes bytes) and synchronises.
 * SIMMR_ESTATE: no simmr_sam_plan for the same columns — every pointer of `reads`, its seq_capacity and layout, and edit_off,
 * edit_pos, edit_ref and edits_capacity of `truth` are the plan's — or a staging call since.  SIMMR_ERANGE, nothing written:
 * dst_capacity < total_bytes.  SIMMR_EINVAL: the CONTENTS of the columns were changed since the plan so that a read fails a check
 * again.  A read refused by the bounds check (names, seq_off, length, edit_off) has its record left unwritten; a read whose
 * edit_pos entries no longer ascend below L is found while its MD is written, and its record is then unspecified — partly
 * written, its MD short — but inside its own bytes.  In both cases no store leaves any record's own bytes. */
int simmr_sam_emit(simmr_engine* e, const simmr_reads_out* reads, const simmr_truth_out* truth,
                   uint8_t* dst, uint64_t dst_capacity);
/* HIP-event time (ms) of the last simmr_sam_plan's device work (size pass + scan) plus that of the simmr_sam_emit after it,
 * if any.  Synchronises the stream. */
int simmr_last_sam_ms(simmr_engine* e, float* ms);

/* ---- the same lines in coordinate order: a stable radix sort of the reads on the device ---------------------------------------
 * What samtools index, IGV, pileup-based callers and gold-standard BAMs want.  Sorting is a permutation of where the records are
 * written, not a second pass over text: (key, read) pairs are sorted, the record sizes scanned in sorted order, and the record
 * writer of simmr_sam_emit puts each line at its sorted offset.
 *
 * Key of read r.  row = the index of (genome[r], contig[r]) among the contigs of `names`, flattened entry by entry: the order in
 * which a caller writes the @SQ lines.  lo = min(start, end).  key = (row << 40) | lo.
 * Order.  Records ascend by key; equal keys ascend by read index r (the sort is stable).  Every read is mapped, so there is no
 * "unmapped last" class; a read with L == 0 sorts by its lo like any other.  Each line's bytes are exactly those simmr_sam_emit
 * writes for that read: the mate fields stay as they are, mates merely stop being adjacent.  The text is a function of the inputs
 * alone: no atomic decides a position and launch geometry changes no byte.
 * Limits.  More than 2^24 named contigs, or a named contig of 2^40 bases or more: SIMMR_ERANGE on the host.  A read whose
 * max(start, end) exceeds the staged length of its contig: refused on the device through the error word (SIMMR_EINVAL), with
 * nothing loaded or stored for it — a check the unsorted calls do not make; it is what bounds the key's width.
 * The sort runs over the significant bits only — bits(longest named contig) + bits(rows - 1) — in 8-bit digits. */

/* The widths of the internal sort key for a names set of n_rows contigs, the longest of longest_contig bases; either pointer may
 * be NULL.  SIMMR_ERANGE: the limits above.  Needs no engine. */
int simmr_sam_sort_key_bits(uint64_t n_rows, uint64_t longest_contig, uint32_t* pos_bits, uint32_t* row_bits);
/* simmr_sam_plan's arguments, checks and status codes, with the limits above on top; *total_bytes is what simmr_sam_plan returns
 * for the same input.  Sizes the records, sorts the reads and scans the sizes in sorted order; the engine holds the result in a
 * state of its own: a sorted plan and an unsorted plan on one engine do not disturb each other. */
int simmr_sam_sort_plan(simmr_engine* e, const simmr_sam_names* names, const simmr_reads_out* reads,
                        const simmr_truth_out* truth, uint64_t n_reads, int paired, uint64_t* total_bytes);
/* simmr_sam_emit's arguments, checks and status codes (the plan meant is the last simmr_sam_sort_plan): the n_reads lines in
 * coordinate order, back to back in dst.  Every store of the i-th line is bounded by that line's planned length, so columns
 * changed since the plan cannot carry a store out of a record.
 * key_out (DEVICE, n_reads entries, may be NULL): the key of the i-th line written.  line_off_out (DEVICE, n_reads + 1 entries,
 * may be NULL): the offset of the i-th line in dst, and total_bytes behind the last.  With them a caller merges several sorted
 * ranges without parsing text. */
int simmr_sam_sort_emit(simmr_engine* e, const simmr_reads_out* reads, const simmr_truth_out* truth,
                        uint8_t* dst, uint64_t dst_capacity, uint64_t* key_out, uint64_t* line_off_out);
/* HIP-event time (ms) of the last simmr_sam_sort_plan's device work (sizes and keys, the sort passes, the scan) plus that of the
 * simmr_sam_sort_emit after it, if any.  Synchronises the stream. */
int simmr_last_sam_sort_ms(simmr_engine* e, float* ms);

/* ---- the true alignments as BAM records, and BGZF framing of any device buffer ------------------------------------------------
 * The binary form of the SAM line above, in read order: every field but QNAME and MD is a fixed-width integer, the bases are
 * packed two to a byte and the qualities are raw Phred bytes, so a record is about half the bytes of its line and a consumer
 * parses no decimal.  Two orthogonal pieces: simmr_bam_* writes the records of SAM spec 4.2 back to back, unframed;
 * simmr_bgzf_frame wraps any device buffer into BGZF blocks.  The blocks hold STORED deflate blocks (compression level 0, what
 * `samtools view -u` writes): every htslib tool reads them, samtools sort / index and bgzip recompress them.  Deflate is
 * deliberately out of scope.  A BAM file is BGZF(header of the host + records) followed by the 28 bytes SIMMR_BGZF_EOF.
 *
 * Record of read r, little-endian, no alignment assumed.  lo, hi, L, rev, FLAG, the mate fields and the MD string are those of
 * the SAM record above; nd = the number of decimal digits of read_id[r]; n = edit_off[r + 1] - edit_off[r].
 *   offset  bytes  field
 *        0      4  block_size   the bytes of the record that follow this field
 *        4      4  refID        the index of (genome[r], contig[r]) among the contigs of `names`, flattened entry by entry: the
 *                               `row` of simmr_sam_sort_*, the order of the @SQ lines
 *        8      4  pos          lo (0-based)
 *       12      1  l_read_name  nd + 1
 *       13      1  mapq         255
 *       14      2  bin          reg2bin(lo, L ? hi : lo + 1) of SAM spec 5.3, the 16 bits the field holds
 *       16      2  n_cigar_op   L ? 1 : 0
 *       18      2  flag         FLAG
 *       20      4  l_seq        L
 *       24      4  next_refID   paired: refID; else -1
 *       28      4  next_pos     paired: lo of read r^1; else -1
 *       32      4  tlen         paired: the signed span of the SAM rule; else 0
 *       36  nd + 1 read_name    read_id[r] in decimal, NUL
 *        .   0 | 4 cigar        L << 4 | 0 (the M operation); no word for L == 0
 *        . (L+1)/2 seq          the bytes SAM shows (forward strand, every byte outside ACGTN as N), 4 bits each: A 1, C 2, G 4, T 8,
 *                               N 15; the earlier base in the high nibble; the low nibble of a last odd byte is 0
 *        .      L  qual         max(byte, 33) - 33 per base, back to front for a rev read
 *        .  4 | 5  NM           'N' 'M' 'C' and n in one byte for n <= 255, else 'N' 'M' 'S' and n in two bytes (n <= L <= 65 535)
 *        .      .  MD           'M' 'D' 'Z', the MD string, NUL
 * Both layouts are read; reads->qual_offset must be 33.
 *
 * The records are a function of the inputs alone: sizes are counted and scanned, records written at their offsets; no atomic
 * hands out space and launch geometry changes no byte.  The size pass and the write pass are one routine.  No store of record r
 * leaves its own bytes of dst even when the columns were changed between the plan and the emit, and no load leaves a read's own
 * bytes of seq[] / qual[] in either layout.
 * Limits: read order and no index here (simmr_bam_sort_* and simmr_bai_* below give coordinate order and a .bai), no @RG. */

/* simmr_sam_plan's arguments, checks and status codes; *record_bytes is the sum of the records' lengths.  On top of them: a read
 * with max(start, end) >= 2^31 is refused on the device through the error word (SIMMR_EINVAL; pos and the read's end are int32),
 * with nothing loaded or stored for it, and more than 2^31 - 1 name rows are SIMMR_ERANGE, decided on the host.  The state is
 * the engine's own for BAM: a BAM plan and a SAM plan on one engine do not disturb each other. */
int simmr_bam_plan(simmr_engine* e, const simmr_sam_names* names, const simmr_reads_out* reads,
                   const simmr_truth_out* truth, uint64_t n_reads, int paired, uint64_t* record_bytes);
/* simmr_sam_emit's arguments, checks and status codes (the plan meant is the last simmr_bam_plan): the n_reads records back to
 * back in dst (DEVICE memory of at least record_bytes bytes), unframed.  Synchronises. */
int simmr_bam_emit(simmr_engine* e, const simmr_reads_out* reads, const simmr_truth_out* truth,
                   uint8_t* dst, uint64_t dst_capacity);
/* HIP-event time (ms) of the last simmr_bam_plan's device work (size pass + scan) plus that of the simmr_bam_emit after it, if
 * any.  Synchronises the stream. */
int simmr_last_bam_ms(simmr_engine* e, float* ms);

/* BGZF (SAM spec 4.1).  src is cut into blocks of 65 280 bytes (0xff00, htslib's figure), the last one shorter; block b of n
 * source bytes starts at byte 65 311 b of dst and is n + 31 bytes:
 *   offset  bytes
 *        0      4  1f 8b 08 04       gzip: magic, deflate, FEXTRA
 *        4      4  00 00 00 00       MTIME
 *        8      2  00 ff             XFL, OS unknown
 *       10      2  06 00             XLEN 6
 *       12      4  'B' 'C' 02 00     the BGZF subfield, 2 bytes long
 *       16      2  BSIZE             n + 30: the block's length - 1
 *       18      1  01                one stored deflate block, the last (BFINAL 1, BTYPE 00)
 *       19      2  LEN               n
 *       21      2  ~LEN
 *       23      n  the bytes
 *   23 + n      4  CRC-32 of the bytes (zlib's: polynomial 0xEDB88320, start value and final xor 0xffffffff)
 *   27 + n      4  ISIZE             n
 * The end-of-file marker is a constant the caller appends, SIMMR_BGZF_EOF:
 *   1f 8b 08 04 00 00 00 00 00 ff 06 00 42 43 02 00 1b 00 03 00 00 00 00 00 00 00 00 00 */
#define SIMMR_BGZF_EOF_BYTES 28
#define SIMMR_BGZF_EOF "\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00\x42\x43\x02\x00\x1b\x00\x03\x00\x00\x00\x00\x00\x00\x00\x00\x00"
/* n_bytes + 31 * ceil(n_bytes / 65 280): what simmr_bgzf_frame writes for n_bytes.  Needs no engine. */
uint64_t simmr_bgzf_bound(uint64_t n_bytes);
/* Frames the n_bytes at src (DEVICE) into dst (DEVICE); *written = simmr_bgzf_bound(n_bytes).  A workgroup takes a block:
 * every lane copies a segment of it and runs a table-driven CRC over it, and the lanes' CRCs are folded with multiplications
 * by x^(8k) mod P.  Synchronises.  n_bytes == 0 writes nothing (*written = 0).  SIMMR_ERANGE, nothing written: dst_capacity is
 * below the bound.  SIMMR_EINVAL: a NULL buffer, or src and dst overlap. */
int simmr_bgzf_frame(simmr_engine* e, const uint8_t* src_device, uint64_t n_bytes, uint8_t* dst_device,
                     uint64_t dst_capacity, uint64_t* written);

/* ---- the BAM records in coordinate order, and the BAI index of a coordinate-sorted record stream ------------------------------
 * What a genome browser, a region query and a caller open directly.  The records are those of simmr_bam_emit, byte for byte; only
 * their places differ: the key and the order are those of simmr_sam_sort_* (key = row << 40 | lo, ties in read order, the stable
 * radix sort of that unit), with its limits and its refusal of a read that ends behind the staged length of its contig.
 *
 * The state of these calls is an object of its own, created on an engine and destroyed BEFORE the engine; its calls run on the
 * engine's stream and leave their messages with the engine (simmr_last_error).  One object holds one sorted plan and one index
 * plan; they do not disturb the engine's own BAM and SAM plans. */
typedef struct simmr_bam_sort simmr_bam_sort;
int simmr_bam_sort_create(simmr_engine* e, simmr_bam_sort** out);
void simmr_bam_sort_destroy(simmr_bam_sort* h);
/* simmr_bam_plan's arguments, checks and status codes, with the limits of simmr_sam_sort_plan on top; *record_bytes is what
 * simmr_bam_plan returns for the same input.  Sizes the records, sorts the reads, scans the sizes in sorted order. */
int simmr_bam_sort_plan(simmr_bam_sort* h, const simmr_sam_names* names, const simmr_reads_out* reads,
                        const simmr_truth_out* truth, uint64_t n_reads, int paired, uint64_t* record_bytes);
/* simmr_bam_emit's arguments, checks and status codes (the plan meant is the handle's last simmr_bam_sort_plan): the n_reads
 * records in coordinate order, back to back in dst, unframed.  Every store of the i-th record is bounded by its planned length.
 * Three optional outputs (DEVICE, may be NULL), all in the order written — what a merge of several sorted ranges and
 * simmr_bai_plan take:
 *   key_out      n_reads entries: the key (row << 40 | lo) of the i-th record, as simmr_sam_sort_emit gives it;
 *   rec_off_out  n_reads + 1 entries: the offset of the i-th record in dst, and record_bytes behind the last;
 *   end_out      n_reads entries: the exclusive end of the reference interval from which the record's own `bin` field was
 *                computed (lo + L, or lo + 1 for a read without bases), so an index built from it cannot disagree with the record. */
int simmr_bam_sort_emit(simmr_bam_sort* h, const simmr_reads_out* reads, const simmr_truth_out* truth,
                        uint8_t* dst, uint64_t dst_capacity, uint64_t* key_out, uint64_t* rec_off_out, uint32_t* end_out);
/* HIP-event time (ms) of the handle's last simmr_bam_sort_plan's device work plus that of the simmr_bam_sort_emit after it, if
 * any.  Synchronises the stream. */
int simmr_last_bam_sort_ms(simmr_bam_sort* h, float* ms);
/* The staged length of every row of the handle's last simmr_bam_sort_plan (HOST, capacity entries; *n_rows = the rows), in the
 * order of the @SQ lines: what the BAM header needs.  SIMMR_ERANGE (with *n_rows set): capacity < the rows. */
int simmr_bam_sort_ref_lengths(simmr_bam_sort* h, uint64_t* lengths, uint64_t capacity, uint64_t* n_rows);

/* The BAI index (SAM spec 5.2) of a coordinate-sorted record stream, built from columns: the file is never read back.
 * Input (DEVICE): key[n] = row << 40 | lo ascending, end[n] (exclusive, lo < end <= 2^29), rec_off[n + 1] non-decreasing — the
 * outputs of simmr_bam_sort_emit, or a merge of several — and on the host n_ref, ref_len[n_ref] (may be NULL: lengths unknown) and
 * `base`, the uncompressed bytes in front of record 0 (the BAM header).
 * Contract on the caller: header and records are framed as ONE stream by simmr_bgzf_frame, so every block but the last holds
 * 65 280 source bytes and the virtual offset of uncompressed position p is ((p / 65280) * 65311) << 16 | (p % 65280), also for p =
 * the stream's length (the EOF block).
 * The file is a pure function of the input:
 *   magic "BAI\1", n_ref; a reference without records has n_bin = 0 and n_intv = 0;
 *   bins      ascending by bin number; a record's bin is reg2bin(lo, end);
 *   chunks    of a bin: the maximal runs of records consecutive in file order that fall into the bin, in file order, each from
 *             the virtual offset of its first record's start to that of its last record's end.  Chunks are not merged across
 *             a gap (htslib merges chunks that share a block; the specification does not ask for it);
 *   bin 37450 behind the real bins of a reference with records (n_bin counts it): two chunks, (virtual offset of the
 *             reference's first record, that behind its last) and (n_mapped, n_unmapped = 0);
 *   linear    n_intv = 1 + ((largest end - 1) >> 14); ioffset[w] = the smallest virtual offset of the start of a record that
 *             overlaps window w of 16 384 bases; a window no record overlaps takes the value of the window before it, 0 at the front;
 *   n_no_coor 0.
 * ref_len == NULL: no length is checked — a contig of 2^29 bases or more is then NOT refused as such, only a record that ends
 * beyond 2^29 is; a caller that knows the lengths passes them.
 * simmr_bai_plan: *bai_bytes = the file's size.  SIMMR_ERANGE: a ref_len of 2^29 or more (CSI is not written), a record that
 * ends beyond 2^29, a stream whose compressed size leaves the 48 bits of a virtual offset, 2^31 records or more, more than 2^24
 * references.  SIMMR_EINVAL: keys that descend, rec_off that decreases, a row >= n_ref, an empty interval — found on the device.
 * simmr_bai_emit writes the file to dst (DEVICE) from the columns of the plan, which must still be there and unchanged; every
 * store is bounded by the plan's layout.  SIMMR_ESTATE without a plan, SIMMR_ERANGE for dst_capacity < bai_bytes.  Both synchronise. */
int simmr_bai_plan(simmr_bam_sort* h, const uint64_t* key, const uint32_t* end, const uint64_t* rec_off, uint64_t n,
                   uint64_t n_ref, const uint64_t* ref_len, uint64_t base, uint64_t* bai_bytes);
int simmr_bai_emit(simmr_bam_sort* h, uint8_t* dst, uint64_t dst_capacity);

/* ---- the true read-to-read overlaps as PAF: which reads of a run share reference bases, found and formatted on the device ------
 * Replaces nothing in the reference.  What overlappers (minimap2 -x ava-ont) and the overlap stage of long-read assemblers are
 * scored against: every pair of reads whose reference intervals share at least min_overlap bases, known here without aligning
 * anything.  The pass needs the metadata columns of simmr_reads_out only — no read byte is loaded — and follows the
 * accumulate-then-read shape of simmr_depth_* and simmr_pileup_*: reads of different ranges of a run overlap too.
 *
 * Definitions.  The row of a read is the index of (genome slot, contig) among all contigs staged on the engine, slots ascending
 * and contigs in staged order (the order simmr_depth_contig_first uses).  lo = min(start, end), hi = max(start, end), L = hi - lo,
 * rev = flags & SIMMR_FLAG_REVCOMP.  The ordinal of a read is its index in the order the reads were added since the reset.  The key
 * is (row << 40) | lo, with the limits of simmr_sam_sort_key_bits (the pass keeps one row value for itself: fewer than 2^24 contigs).
 * Place order ascends by key, equal keys by ordinal — among the reads with L >= min_overlap; the reads with L < min_overlap take the
 * places behind all of those, in ordinal order (they are in no record, so the order of the records is not touched by where they lie).
 *
 * The overlap.  Reads a and b overlap when they share a row and ov = min(hi_a, hi_b) - max(lo_a, lo_b) >= min_overlap >= 1.  Every
 * unordered pair is reported once: the query is the read at the earlier place, the target the read at the later place, and records
 * are ordered by (place of the query, place of the target).  Mates of one pair are reads like any others and may overlap each other.
 * A read with L < min_overlap is in no record.
 *
 * The record: twelve tab-separated PAF columns and '\n':
 *   query name, L_q, query start, query end, '+' if rev_q == rev_t else '-', target name, L_t, target start, target end, ov, ov, 255
 * The name is read_id in decimal; when the reset said `paired` it is followed by /1 or /2 by the parity of the read's index within
 * its add call.  Start and end are the shared reference interval [s, e) = [max(lo), min(hi)) in the read's own as-written
 * coordinates: [s - lo, e - lo) for a forward read, [hi - e, hi - s) for a rev read.  Columns 10 and 11 both carry the length of
 * the shared reference interval: the record is a fact about where the reads came from, not an alignment of their bases (which may
 * differ by the profile's substitutions).  No profile changes a read's length, so there are no gaps.
 *
 * The output is a function of the inputs alone: partners are counted and scanned, record sizes counted and scanned, and every record
 * written at its offset; no atomic hands out space and launch geometry changes no byte.  No store leaves dst[0, bytes) or a column's
 * own entries. */
typedef struct simmr_overlap_cols {   /* DEVICE pointers, caller-owned; any column may be NULL.  One entry per record */
  uint32_t* a;          /* ordinal of the query  */
  uint32_t* b;          /* ordinal of the target */
  uint64_t* ref_start;  /* s: the shared reference interval inside the contig */
  uint64_t* ref_end;    /* e */
  uint32_t* row;        /* the row both reads lie on */
  uint64_t capacity;    /* entries available in every column given */
} simmr_overlap_cols;
/* Drops what was accumulated (and any plan) and fixes the rows to what is staged now; `paired`: the reads of every add call are
 * interleaved mates, named /1 and /2.  Synchronises.  SIMMR_ERANGE: 2^24 contigs or more, or a contig of 2^40 bases or more. */
int simmr_overlap_reset(simmr_engine* e, int paired);
/* Appends (key, L, read_id, rev, mate bit) of every read to engine-held columns that grow (20 bytes a read).  Needs start, end,
 * contig, genome, read_id and flags; seq, qual and seq_off are never read.  Synchronises, and drops the plan in force.
 * SIMMR_EINVAL: a missing column, an odd n_reads under `paired`; and, found on the device and reported through an error word with
 * nothing appended for the call: a read whose genome slot or contig is not staged, or whose hi exceeds the contig's staged length.
 * SIMMR_ERANGE: the reads added since the reset would reach 2^31.  SIMMR_ESTATE: no simmr_overlap_reset yet, or a staging call
 * since the reset. */
int simmr_overlap_add(simmr_engine* e, const simmr_reads_out* reads, uint64_t n_reads);
/* Sorts the reads added, counts the partners of every place, sizes every record, scans both, and keeps the result until the next
 * add or reset.  *n_reads: the places (every read added has one); *n_pairs: the records; *total_bytes: their text.  Any of the
 * three pointers may be NULL.  SIMMR_EINVAL: min_overlap == 0.  SIMMR_ESTATE: as simmr_overlap_add. */
int simmr_overlap_plan(simmr_engine* e, uint64_t min_overlap, uint64_t* n_reads, uint64_t* n_pairs, uint64_t* total_bytes);
/* The longest run of places from first_place (<= n_reads) whose records fit max_bytes: its places, records and bytes.  A place
 * without records fits anywhere.  SIMMR_ERANGE: the first place alone does not fit; *bytes then holds what it needs and *n_places
 * is 0.  With this a caller drains an output larger than its buffer in pieces: emit the run, go on at first_place + n_places, until
 * that is n_reads.  SIMMR_ESTATE: no simmr_overlap_plan for the reads added, or a staging call since the reset. */
int simmr_overlap_window(simmr_engine* e, uint64_t first_place, uint64_t max_bytes, uint64_t* n_places, uint64_t* n_pairs,
                         uint64_t* bytes);
/* Writes the records whose query place is in [first_place, first_place + n_places): the text back to back into dst (DEVICE), the
 * columns of the same records into `cols`.  Either of dst and cols may be NULL, and so may any column.  Synchronises.
 * SIMMR_ERANGE, nothing written: dst_capacity is below the run's bytes, or cols->capacity below its records.  SIMMR_EINVAL: the run
 * leaves the places.  SIMMR_ESTATE: as simmr_overlap_window. */
int simmr_overlap_emit(simmr_engine* e, uint64_t first_place, uint64_t n_places, const simmr_overlap_cols* cols, uint8_t* dst,
                       uint64_t dst_capacity);
/* HIP-event time (ms) of the last simmr_overlap_plan's device work plus that of the simmr_overlap_emit calls since.  Synchronises
 * the stream. */
int simmr_last_overlap_ms(simmr_engine* e, float* ms);

/* ---- fitting an error model from a run: what `simmrd` makes from alignments, counted on the device ----------------
 * The reference's second program builds a shared::encoding::ErrorModelParams from SAM records: k-mer to alternate-k-mer
 * probabilities, a quality density per read offset, read-length and insert-size densities.  Here the same products come
 * from the columns of a run in HBM: the bases as written, the expected bases from the staged planes, the qualities.
 *
 * Definitions.  The EXPECTED byte, the WRITTEN byte, the quality q, L, the layouts (compact and SIMMR_SLOT16), the set
 * r % n_sets and the bounds check are exactly simmr_stats_add's (above).  Everything is in the READ'S OWN orientation,
 * reverse mates complemented: the orientation in which the custom profiles consume a model.  (The reference reverse-
 * complements SEQ and then applies the forward CIGAR / MD to it, and skips a second record with a name already seen:
 * accidents of its SAM route, not reproduced.)
 *
 * K-mer pairs (simmrd/src/alignment.rs, encoded_kmerize_alignment, for an alignment without gaps).  For every read and
 * every ndx with ndx + k < L (strictly: the last window is left out, as in the reference) the reference k-mer is
 * expected[ndx .. ndx + k).  A byte of it outside A C G T (a staged N or '-') skips the window.  The query k-mer is
 * written[ndx .. ndx + k) with every N and '-' removed and N appended back to length k; nothing left skips the window,
 * and so does a written byte outside A C G T N '-' (the reference's encoder refuses it).  Both are 3-bit coded, base i at
 * bits 3 i, A C G T N = 0 1 2 3 4.  The window adds 1 to count[ref][ref] and 1 to count[ref][query]: an unchanged window
 * adds 2 to count[ref][ref].  k is 3 .. 10, counts are 64-bit.  Per reference k-mer: total = the sum over its alternates,
 * probability = (float)count / (float)total in f32 (the 64-bit values converted; the reference's u32 counts end at 2^32,
 * which is documented, not emulated), alternates by count descending, ties by code ascending, cut to the first
 * max_alt_kmers WITHOUT renormalising, as in the reference.  Reference k-mers ascend by code (the reference's order is its
 * HashMap's).
 *
 * Qualities.  hist[pos][q] for every offset pos < L of every read, q = 0 .. SIMMR_FIT_MAX_Q (a larger q sets the sticky
 * error); positions run to the longest read seen (no 512-cycle limit).  Per position, over its n observations: population
 * mean and standard deviation (shared/src/util.rs), bandwidth 1.06 sd n^(-1/5), and density[s] for s = 0 .. 70 by
 * probability.rs's `gaussian`: SIMMR_FIT_DENSITIES = 71 values beside num_bins = 70 and 70 bin_ranges (i, i), as the
 * reference writes them.  All in f64, summed over histogram entries, not observations.
 *
 * Read lengths.  A histogram of L over all reads; mean, standard deviation, is_long = mean > 400; the bin width by
 * freedman_diaconis_rule with the quartiles read from the cumulative histogram at indices floor(n * 0.25) and
 * floor(n * 0.75), (2 iqr / n^(1/3)) as usize, 10 if that is <= 1; bins, clamped ends and mid-point densities as
 * create_read_length_bins.
 * Insert sizes (n_sets == 2 only).  For each mate |TLEN| as the SAM pass defines TLEN for the pair (the span of the two
 * mates), pushed once per mate as the reference pushes it once per record; values above SIMMR_FIT_MAX_INSERT are left
 * out.  Mean, standard deviation and bins as create_insert_size_bins (ends not clamped; the quartiles are those of the
 * sorted values, where the reference indexes its unsorted list).  No insert bins when is_long or when nothing was kept
 * (the mean and the deviation are then 0, where the reference writes NaN).
 *
 * One deliberate departure.  A bandwidth of 0 (every observation equal: one observation, perfect-short's constant Phred,
 * a constant read length) makes the reference divide by zero and write NaN, which its own loader then rejects.  Here
 * the density is the point mass: 1.0 at that value and 0.0 elsewhere, a quality above 70 going to entry 70; a length or
 * insert column with min == max gets ONE bin (min, min) of density 1.0 (the reference gives zero bins).
 *
 * Every table is an integer sum over reads: identical for any launch geometry, layout or split into adds.  The finish
 * runs on the device too (the pairs sorted, totalled, cut and divided; the densities evaluated); the host takes only the
 * scalars and the bins of the length and insert histograms. */
#define SIMMR_FIT_MAX_Q 93u          /* largest quality taken */
#define SIMMR_FIT_QUALS 94u          /* entries of a position's quality histogram */
#define SIMMR_FIT_DENSITIES 71u      /* entries of a position's binned_density */
#define SIMMR_FIT_MAX_L 65535u       /* longest read taken; the length histogram has SIMMR_FIT_MAX_L + 1 entries */
#define SIMMR_FIT_MAX_INSERT 5000u   /* largest insert kept; the insert histogram has SIMMR_FIT_MAX_INSERT + 1 entries */

typedef struct simmr_fit_info {      /* HOST memory: the sizes and scalars of the model simmr_fit_plan made */
  uint64_t n_ref_kmers;              /* reference k-mers */
  uint64_t n_pairs;                  /* (reference, alternate) pairs kept after the cut */
  uint64_t n_positions;              /* the longest read seen */
  uint64_t n_length_bins;
  uint64_t n_insert_bins;            /* 0: insert_size_bins is absent */
  uint64_t n_reads;                  /* observations of the length histogram */
  uint64_t n_inserts;                /* observations of the insert histogram */
  uint64_t length_bin_width;
  uint64_t insert_bin_width;
  double read_length_mean, read_length_std;
  double insert_size_mean, insert_size_std;
  uint32_t is_long;
  uint32_t k;
  uint32_t max_alt_kmers;
  uint32_t pad;
} simmr_fit_info;

typedef struct simmr_fit_out {       /* DEVICE pointers, caller-owned; any column may be NULL */
  uint32_t* kmer_ref;                /* [n_ref_kmers] 3-bit codes, ascending */
  uint64_t* kmer_first;              /* [n_ref_kmers + 1]: the pairs of reference k-mer i are kmer_first[i] .. kmer_first[i + 1] - 1 */
  uint32_t* pair_alt;                /* [n_pairs] */
  uint64_t* pair_count;              /* [n_pairs] */
  float* pair_prob;                  /* [n_pairs] */
  uint64_t* qual_hist;               /* [n_positions][SIMMR_FIT_QUALS] */
  double* qual_density;              /* [n_positions][SIMMR_FIT_DENSITIES] */
  uint64_t* length_hist;             /* [SIMMR_FIT_MAX_L + 1] */
  uint64_t* insert_hist;             /* [SIMMR_FIT_MAX_INSERT + 1] */
  double* length_density;            /* [n_length_bins] */
  uint32_t* length_lo;               /* [n_length_bins] bin_ranges .0 */
  uint32_t* length_hi;               /* [n_length_bins] bin_ranges .1 */
  double* insert_density;            /* [n_insert_bins] */
  uint32_t* insert_lo;
  uint32_t* insert_hi;
  uint64_t ref_capacity;             /* entries available in kmer_ref (kmer_first has one more) */
  uint64_t pair_capacity;            /* ... in the three pair columns */
  uint64_t position_capacity;        /* positions available in qual_hist and qual_density */
  uint64_t length_bin_capacity;
  uint64_t insert_bin_capacity;
} simmr_fit_out;

/* Allocates the tables on first use and zeroes them and the sticky error.  pair_capacity: how many distinct CHANGED
 * (reference, alternate) pairs the run may show; the open-addressing table gets the next power of two at or above twice
 * that.  SIMMR_EINVAL: k outside 3 .. 10, max_alt_kmers == 0, pair_capacity == 0 or above 2^26. */
int simmr_fit_reset(simmr_engine* e, uint32_t k, uint32_t max_alt_kmers, uint64_t pair_capacity);
/* Adds the reads of `reads`.  Only enqueues on the engine's stream; can be called once per range.  Needs seq, qual,
 * seq_off, start, end, contig, genome and flags.  Staging a genome afterwards does not discard the tables (the rule of
 * simmr_stats_add), but the genomes the columns name must be staged when the add runs.
 * SIMMR_EINVAL, at once: n_sets other than 1 or 2, an odd n_reads with n_sets == 2, a missing column.  SIMMR_ESTATE: no
 * simmr_fit_reset yet.  Sticky, reported by simmr_fit_plan: a read that fails simmr_stats_add's bounds check (unstaged
 * genome or contig, a window out of bounds, L > SIMMR_FIT_MAX_L), q > SIMMR_FIT_MAX_Q, a full pair table. */
int simmr_fit_add(simmr_engine* e, const simmr_reads_out* reads, uint64_t n_reads, uint32_t n_sets);
/* Finishes the model from what was added since the reset, keeps it for simmr_fit_emit, synchronises and fills *info.
 * Adds may follow; the next plan takes them in.  SIMMR_EINVAL (nothing made): the sticky error of a bad read or quality.
 * SIMMR_ERANGE: the pair table was full.  SIMMR_ESTATE: no simmr_fit_reset yet. */
int simmr_fit_plan(simmr_engine* e, simmr_fit_info* info);
/* Copies the planned model into the columns given.  Synchronises.  SIMMR_ERANGE (nothing written): a capacity below its
 * size in simmr_fit_info.  SIMMR_ESTATE: no simmr_fit_plan since the last reset or add. */
int simmr_fit_emit(simmr_engine* e, const simmr_fit_out* out);
/* HIP-event time (ms) of the last simmr_fit_add's device work.  Synchronises the stream. */
int simmr_last_fit_ms(simmr_engine* e, float* ms);

/* ---- the same fit from a user's SAM file: text in HBM, parsed on the device ------------------------------------------
 * What `simmrd` itself starts from (simmrd/src/main.rs:110-260, simmrd/src/alignment.rs): SAM records with CIGAR and
 * MD:Z.  simmr_fit_add_sam adds the records of `text` into the SAME tables as simmr_fit_add, so adds from columns and from
 * SAM may be mixed between one simmr_fit_reset and one simmr_fit_plan; no genome need be staged.  The SAM text of a run
 * (simmr_sam_emit, either order) gives the model of that run's columns, byte for byte.
 *
 * Text.  Whole lines of plain SAM (no BAM, no gzip): every line ends in '\n', except that the last line of a call may lack
 * it; the caller cuts a large file at line ends, at most SIMMR_FIT_SAM_MAX_BYTES a call.  An empty line is skipped and not
 * counted.  A line that starts with '@' is a header line: counted and skipped.  Every other line is a record of tab-separated
 * fields: 11 mandatory ones and the optional ones, of which the first that starts with "MD:Z:" is taken.
 *
 * Malformed (sticky, simmr_fit_plan answers SIMMR_EINVAL and makes nothing): a record with fewer than 11 fields; a FLAG,
 * MAPQ or TLEN that is not a decimal number (1 to 18 digits; TLEN may start with '-'); a CIGAR that is neither "*" nor
 * (<digits><op>)+ with 1 to 9 digits a run, an op being any byte that is no digit; a QUAL that is neither "*" nor exactly as
 * long as SEQ (a SEQ of "*" has no bases: its QUAL is "*"); a QUAL byte outside '!' .. '~'.  These are checked on every
 * record, whatever the filters would say of it.
 *
 * Filters, in this order (main.rs:156-232); L = the length of SEQ, the quality of a byte is byte - 33:
 *    1. SEQ is "*": skip_no_sequence.
 *    2. FLAG has 0x100 or 0x800: skip_secondary.  (This stands in for the reference's "name already seen", which also drops
 *       every mate 2 whose name equals mate 1's: the accident noted above, not reproduced.)
 *    3. L > SIMMR_FIT_MAX_L: skip_too_long.
 *    4. The record counts for the length histogram and, if QUAL is not "*", for the quality histogram (taken_quality).
 *    5. FLAG 0x4: skip_unmapped.                        6. MAPQ == 0: skip_mapq0 (255 passes, as in the reference).
 *    7. n_sets == 2, TLEN == 0 and FLAG 0x8: skip_mate_unmapped.           8. No MD:Z: field: skip_no_md.
 *    9. n_sets == 2 and |TLEN| > SIMMR_FIT_MAX_INSERT: skip_insert.
 *   10. n_sets == 2: |TLEN| goes into the insert histogram (n_sets == 1 takes no inserts: simmr_fit_add's rule).
 *   11. The alignment is taken (taken_alignment), unless the next paragraph skips it; that does not undo steps 4 and 10.
 *
 * Alignment rows (alignment.rs, reconstruct_alignment), built in SAM's forward orientation.  M, = and X give one column
 * each: the query byte from SEQ, the reference byte that same byte where MD says match and MD's letter where it says
 * mismatch.  I: reference '-', the query byte.  D: the reference byte from MD's '^' run, query '-'.  H: nothing.  S consumes
 * query bases and gives NO column — a departure: the reference walks MD through soft clips, which MD does not cover, and
 * so shifts every later base.  N, P, any other op, or a CIGAR of "*": skip_cigar_op (the reference panics).  MD is numbers of
 * 1 to 9 digits, letters 'A' .. 'Z' and '^'; a letter is a deleted base when the nearest byte before it that is no letter
 * is '^', otherwise a mismatch.  skip_inconsistent, where the reference would silently truncate: the query bases of the
 * CIGAR (M = X I S) differ from L; MD's matches plus mismatches differ from the CIGAR's M = X columns; MD's deleted bases
 * differ from its D columns; MD holds another byte or a longer number.
 *
 * Orientation.  With FLAG 0x10 both rows are reversed and complemented (A <-> T, C <-> G; a gap and every other byte keep
 * their byte), and quality offset i of the read is QUAL[L - 1 - i]: the read's own orientation, what simmr_fit_add counts in
 * and what the custom profiles consume.  A departure beside the one above: the reference complements SEQ and keeps the forward
 * CIGAR, and indexes qualities in file order.
 *
 * Windows.  The k-mer rule above over the two rows, with `columns` (M = X + I + D) in the place of L: every ndx with
 * ndx + k < columns, over k COLUMNS.  A reference window that holds a '-' or a byte outside ACGT is skipped; the query
 * window loses its '-' and N and is N-padded; an empty query window, or a query byte outside ACGTN-, is skipped.
 *
 * Every table stays an integer sum over records: the same for any launch geometry and any cut of the text into adds. */
#define SIMMR_FIT_SAM_MAX_BYTES 0xf0000000ull   /* most bytes of text in one simmr_fit_add_sam */

typedef struct simmr_fit_sam_counts {   /* HOST; every entry an integer sum over lines, cumulative since simmr_fit_reset */
  uint64_t lines, header_lines, records;   /* lines = header_lines + records: empty lines are not counted */
  uint64_t taken_quality;      /* records whose length (and qualities, if present) were counted */
  uint64_t taken_alignment;    /* records whose k-mer windows were counted */
  uint64_t skip_no_sequence, skip_secondary, skip_too_long, skip_unmapped, skip_mapq0,
           skip_mate_unmapped, skip_no_md, skip_insert, skip_cigar_op, skip_inconsistent;
} simmr_fit_sam_counts;

/* Adds the records of text[0 .. n_bytes) (DEVICE memory, which must stay as it is until the stream has run the add).  Only
 * enqueues on the engine's stream; timed by simmr_last_fit_ms like simmr_fit_add.  Side buffers of about seven bytes per byte
 * of text grow with the engine and are freed with it.
 * SIMMR_EINVAL, at once: n_sets other than 1 or 2, a NULL text with n_bytes > 0.  SIMMR_ENOTSUP: n_bytes above
 * SIMMR_FIT_SAM_MAX_BYTES.  SIMMR_ESTATE: no simmr_fit_reset yet.  Sticky, reported by simmr_fit_plan as SIMMR_EINVAL: a
 * malformed record (above); SIMMR_ERANGE there: a full pair table. */
int simmr_fit_add_sam(simmr_engine* e, const uint8_t* text, uint64_t n_bytes, uint32_t n_sets);
/* The counts of the SAM adds since the last simmr_fit_reset.  Synchronises.  SIMMR_ESTATE: no simmr_fit_reset yet. */
int simmr_fit_sam_counts_read(simmr_engine* e, simmr_fit_sam_counts* out);

/* ---- an aligner's SAM scored against the true alignments: two texts in HBM, joined and classified on the device ---------------
 * Replaces nothing in the reference.  What a simulator with ground truth is bought for, and what wgsim_eval and paftools mapeval
 * do on the host: how many reads an aligner placed correctly, at which mapping quality.  Two SAM texts go in — the truth (the
 * text of simmr_sam_emit, either order, or any SAM that follows the rules below) and the aligner's output for the same reads —
 * and integer tables come out.  No simulation, no genome: like simmr_fit_add_sam.
 *
 * Text.  The rules of simmr_fit_add_sam: whole lines of plain SAM, every line ends in '\n' except that the last line of a call
 * may lack it; the caller cuts a file at line ends, at most SIMMR_FIT_SAM_MAX_BYTES a call; an empty line is skipped and not
 * counted; a line that starts with '@' is a header line, counted and skipped.  Every other line is a record.
 *
 * Malformed (sticky; simmr_mapeval_read answers SIMMR_EINVAL, simmr_mapeval_truth_plan too for the truth), checked on every
 * record before any filter: fewer than 11 fields; a FLAG, POS or MAPQ that is not a decimal number of 1 to 18 digits; a MAPQ
 * above 255; a POS above 2^31 - 1; a CIGAR that is neither "*" nor (<digits><op>)+ with 1 to 9 digits a run, an op being any
 * byte that is no digit; an interval (below) that ends above 2^40.  SEQ, QUAL and the optional fields are not read.
 *
 * Key.  QNAME is the read id: 1 to 18 decimal digits (so below 2^62).  mate = (FLAG & 0x80) != 0.  key = id << 1 | mate.
 * Names.  The caller hands in the reference names once (simmr_mapeval_config).  The library keeps them sorted in a device blob;
 * a record's RNAME is resolved by exact byte comparison (a binary search, no hash).  The row of a name is its place in that
 * order; only the equality of rows matters.
 * Interval.  [POS - 1, POS - 1 + M + D), M counting the runs of M, = and X; S, H and I take no reference; a CIGAR of "*" gives
 * the empty interval.  A record with any other op (N, P, ...) is left out: the limit of the fit's SAM route.
 *
 * Truth record, in this order:
 *   1. FLAG has 0x100, 0x800 or 0x4, or the CIGAR holds another op: counted truth_skipped.
 *   2. Malformed on this side: a QNAME that is not a read id, an RNAME outside the names, a POS of 0.
 *   3. An entry: key, name row, interval, strand (FLAG & 0x10).  Counted truth_entries.
 * Aligned record, in this order:
 *   1. FLAG has 0x100 or 0x800: secondary.                  2. The CIGAR holds another op: cigar_op.
 *   3. QNAME is not a read id, or no truth entry has the key: unknown_read.
 *   4. FLAG 0x4, or RNAME "*": class 1, unmapped.
 *   5. Otherwise the record is mapped (a POS of 0 here is malformed).  An RNAME outside the names: unknown_ref, and class 2,
 *      wrong.  Else class 3, correct, iff the name row equals the entry's, the strand (FLAG & 0x10) equals the entry's, and with
 *      ov = the length of the intersection of the two intervals and un = max(ends) - min(starts): ov >= 1 and
 *      100 * ov >= min_overlap_pct * un, in 64-bit integers (min_overlap_pct 10 is the criterion of paftools mapeval).
 *      Every other mapped record is class 2, wrong.  by_mapq[MAPQ][class 3 ? 0 : 1] counts it.
 *   6. Steps 4 and 5 give the entry a hit: hits[entry] += 1, best[entry] = max(best[entry], class << 8 | MAPQ).
 * Every output is an integer sum or maximum: the same for any launch geometry and any cut of either text into adds. */
typedef struct simmr_mapeval simmr_mapeval;

typedef struct simmr_mapeval_config {   /* HOST memory */
  uint32_t n_names;
  uint32_t min_overlap_pct;             /* 1 .. 100; 0: the default, 10 */
  const char* const* rname;             /* n_names reference names, NUL-terminated, in any order */
} simmr_mapeval_config;

typedef struct simmr_mapeval_counts {   /* HOST; every entry an integer sum, in this order */
  uint64_t truth_lines, truth_header, truth_entries, truth_skipped;   /* lines = header + records; cumulative since the reset */
  uint64_t lines, header, records;                                    /* the aligned side, since the last truth plan */
  uint64_t secondary, cigar_op, unknown_read, unknown_ref, unmapped, correct, wrong;   /* unknown_ref records are among wrong */
  uint64_t missing, multiple;           /* truth entries with no hit, with more than one */
  uint64_t reads_correct, reads_wrong, reads_unmapped;   /* truth entries by the class of their best record */
} simmr_mapeval_counts;

/* The state is an object of its own, created on an engine and destroyed BEFORE the engine (as simmr_bam_sort_create); its calls
 * run on the engine's stream and leave their messages with the engine (simmr_last_error). */
int simmr_mapeval_create(simmr_engine* e, simmr_mapeval** out);
void simmr_mapeval_destroy(simmr_mapeval* h);
/* Takes the names and min_overlap_pct, and empties both sides.  SIMMR_EINVAL: a NULL argument, min_overlap_pct above 100, a name
 * given twice.  SIMMR_ENOTSUP: a name that is empty, longer than 254 bytes or no SAM reference name (the rule of
 * simmr_sam_plan).  SIMMR_ERANGE: more than 2^24 names. */
int simmr_mapeval_reset(simmr_mapeval* h, const simmr_mapeval_config* cfg);
/* Adds the records of text[0 .. n_bytes) (DEVICE memory, which must stay as it is until the stream has run the add) to the
 * truth.  Only enqueues.  Drops a truth plan.  Room for an entry per 21 bytes of text (no record is shorter) grows with the
 * object.  SIMMR_ESTATE: no reset yet.  SIMMR_EINVAL: a NULL text with n_bytes > 0.  SIMMR_ENOTSUP: n_bytes above
 * SIMMR_FIT_SAM_MAX_BYTES. */
int simmr_mapeval_truth_add(simmr_mapeval* h, const uint8_t* text, uint64_t n_bytes);
/* Sorts the entries by key (the radix sort of simmr_sam_sort_plan, over the bits of the largest key), checks that no key
 * stands twice, empties the aligned side and synchronises.  *n_entries (may be NULL) = the entries.  SIMMR_EINVAL: a malformed
 * truth record, or two entries with one key.  SIMMR_ERANGE: 2^31 entries or more. */
int simmr_mapeval_truth_plan(simmr_mapeval* h, uint64_t* n_entries);
/* Scores the records of text[0 .. n_bytes) (DEVICE, as above) against the plan.  Only enqueues.  SIMMR_ESTATE: no truth plan
 * in force.  SIMMR_EINVAL, SIMMR_ENOTSUP: as simmr_mapeval_truth_add. */
int simmr_mapeval_add(simmr_mapeval* h, const uint8_t* text, uint64_t n_bytes);
/* The counts and by_mapq_host[256][2] (HOST, either may be NULL): the mapped records by MAPQ, [0] correct and [1] wrong.
 * Synchronises.  The last five counts are made here, by a reduction over best[] and hits[].  SIMMR_EINVAL: a malformed record
 * on either side since the reset (nothing is written).  SIMMR_ESTATE: no reset yet. */
int simmr_mapeval_read(simmr_mapeval* h, simmr_mapeval_counts* counts, uint64_t* by_mapq_host);
/* The truth entries in ascending key order (unique keys: the order is a function of the input), three columns (DEVICE, capacity
 * entries each, any may be NULL): key, best = the maximum over the entry's hits of class << 8 | MAPQ (0: no hit), hits.
 * Synchronises.  SIMMR_ESTATE: no truth plan.  SIMMR_ERANGE, nothing written: capacity < n_entries. */
int simmr_mapeval_emit(simmr_mapeval* h, uint64_t* key_dev, uint32_t* best_dev, uint32_t* hits_dev, uint64_t capacity);
/* HIP-event time (ms) of the device work of every add and plan since the last reset.  Synchronises the stream. */
int simmr_last_mapeval_ms(simmr_mapeval* h, float* ms);

/* ---- an overlapper's PAF scored against the true overlaps: two texts in HBM, joined and classified on the device --------------
 * Replaces nothing in the reference.  The other half of simmr_overlap_*: the truth (the text of simmr_overlap_emit, or any PAF
 * that follows the rules below) and an all-vs-all overlapper's output for the same reads go in, and integer tables come out:
 * the records that are correct and wrong and why, the true pairs found, missed and reported more than once, and found / not
 * found by the true overlap's length.  No simulation, no genome: like simmr_mapeval_*.
 *
 * Text.  Whole lines of plain PAF (no gzip): every line ends in '\n', except that the last line of a call may lack it; the
 * caller cuts a file at line ends, at most SIMMR_FIT_SAM_MAX_BYTES a call.  An empty line is skipped and not counted.  There are
 * no header lines: every other line is a record.
 *
 * Record.  At least 12 tab-separated fields; further fields (tags) are not read:
 *   1 query name, 2 query length, 3 query start, 4 query end, 5 strand, 6 target name, 7 target length, 8 target start,
 *   9 target end, 10 matches, 11 block length, 12 mapping quality.
 * Fields 2, 3, 4 and 7 to 12 are decimal numbers of 1 to 18 digits; field 5 is "+" or "-"; on both sides
 * start <= end <= length < 2^40.
 * Malformed (sticky; simmr_ovleval_read answers SIMMR_EINVAL, simmr_ovleval_truth_plan too for the truth), checked on every
 * record before any filter: anything else in those fields.  A malformed line is counted in truth_lines / lines and not in
 * truth_entries / records.
 *
 * Name and key.  A read name is a read id of 1 to 18 decimal digits, optionally followed by "/1" or "/2": exactly what
 * simmr_overlap_emit writes.  mate = 1 iff the suffix is "/2".  key = id << 1 | mate.
 *
 * Truth record.  Both names must be read names and the two keys must differ; otherwise the record is malformed.  The entry is
 * the unordered pair (lo_key, hi_key), lo_key < hi_key.  It holds the relative strand (field 5), the interval [start, end) of
 * the lower-keyed read and that of the higher-keyed read, each in its own read's coordinates as PAF gives them, and
 * ov = query end - query start.  Two entries with one pair: simmr_ovleval_truth_plan answers SIMMR_EINVAL.  The reads of the
 * truth are the distinct keys of its entries.
 *
 * Candidate record, in this order (records counts every well-formed one):
 *   1. Either name is not a read name, or its key is that of no read of the truth: unknown_read, and the record is wrong.
 *   2. Both keys are equal: self, and the record is left out (neither correct nor wrong).
 *   3. The pair is not an entry: no_pair, wrong.
 *   4. The strand differs from the entry's: wrong_strand, wrong.
 *   5. For each of the two reads the record's interval on that read is compared with the entry's: with ov = the length of the
 *      intersection and un = max(ends) - min(starts), the comparison holds iff ov >= 1 and 100 * ov >= min_pct * un, in 64-bit
 *      integers.  A candidate may name the pair in either order; its query interval goes with whichever read it names as
 *      query.  If either read's comparison fails: wrong_interval, wrong.  Otherwise: correct.
 *   6. Steps 4 and 5 give the entry a hit: hits[entry] += 1, best[entry] = max(best[entry], class), class 2 for wrong and 3 for
 *      correct.
 * wrong = unknown_read + no_pair + wrong_strand + wrong_interval; records = wrong + correct + self.
 * Every output is an integer sum or maximum: the same for any launch geometry and any cut of either text into adds. */
#define SIMMR_OVLEVAL_LEN_ROWS 41u   /* by_len: row b holds the entries whose ov has bit length b (0 for ov == 0; ov < 2^40) */

typedef struct simmr_ovleval simmr_ovleval;

typedef struct simmr_ovleval_counts {   /* HOST; every entry an integer sum, in this order */
  uint64_t truth_lines, truth_entries, truth_reads;   /* cumulative since the reset; truth_reads: the distinct keys, made by the plan */
  uint64_t lines, records;                            /* the candidate side, since the last truth plan */
  uint64_t unknown_read, self, no_pair, wrong_strand, wrong_interval, correct, wrong;
  uint64_t pairs_found, pairs_wrong, pairs_missed, pairs_multiple;   /* truth entries: best 3, best 2, no hit, more than one hit */
} simmr_ovleval_counts;

/* The state is an object of its own, created on an engine and destroyed BEFORE the engine (as simmr_mapeval_create); its calls
 * run on the engine's stream and leave their messages with the engine (simmr_last_error). */
int simmr_ovleval_create(simmr_engine* e, simmr_ovleval** out);
void simmr_ovleval_destroy(simmr_ovleval* h);
/* Takes min_pct (1 .. 100; 0: the default, 10) and empties both sides.  Synchronises.  SIMMR_EINVAL: min_pct above 100. */
int simmr_ovleval_reset(simmr_ovleval* h, uint32_t min_pct);
/* Adds the records of text[0 .. n_bytes) (DEVICE memory, which must stay as it is until the stream has run the add) to the
 * truth.  Only enqueues.  Drops a truth plan.  Room for an entry per 23 bytes of text (no record is shorter) grows with the
 * object.  SIMMR_ESTATE: no reset yet.  SIMMR_EINVAL: a NULL text with n_bytes > 0.  SIMMR_ENOTSUP: n_bytes above
 * SIMMR_FIT_SAM_MAX_BYTES. */
int simmr_ovleval_truth_add(simmr_ovleval* h, const uint8_t* text, uint64_t n_bytes);
/* Ranks the reads (the 2 n keys sorted by the radix sort of simmr_sam_sort_plan, their heads flagged and scanned: a dense rank
 * below 2^31 per distinct key), sorts the entries by rank_lo << 31 | rank_hi, checks that no pair stands twice, empties the
 * candidate side and synchronises.  *n_entries, *n_reads (either may be NULL) = the entries and the distinct keys.
 * SIMMR_EINVAL: a malformed truth record, or two entries with one pair.  SIMMR_ERANGE: 2^30 entries or more. */
int simmr_ovleval_truth_plan(simmr_ovleval* h, uint64_t* n_entries, uint64_t* n_reads);
/* Scores the records of text[0 .. n_bytes) (DEVICE, as above) against the plan.  Only enqueues.  SIMMR_ESTATE: no truth plan
 * in force.  SIMMR_EINVAL, SIMMR_ENOTSUP: as simmr_ovleval_truth_add. */
int simmr_ovleval_add(simmr_ovleval* h, const uint8_t* text, uint64_t n_bytes);
/* The counts and by_len_host[SIMMR_OVLEVAL_LEN_ROWS][2] (HOST, either may be NULL): the truth entries by the bit length of
 * their ov, [0] found (best 3) and [1] not found.  Synchronises.  The pairs_* counts and by_len are made here, by a reduction over
 * best[], hits[] and ov[].  SIMMR_EINVAL: a malformed record on either side since the reset (nothing is written).
 * SIMMR_ESTATE: no reset yet. */
int simmr_ovleval_read(simmr_ovleval* h, simmr_ovleval_counts* counts, uint64_t* by_len_host);
/* The truth entries, five columns (DEVICE, capacity entries each, any may be NULL): key_a < key_b the pair's keys, ov, best (0:
 * no hit, 2: wrong, 3: correct), hits.  Entries ascend by (key_a, key_b): ranks are monotone in keys, so this is the sorted
 * order, a function of the input.  Synchronises.  SIMMR_ESTATE: no truth plan.  SIMMR_ERANGE, nothing written:
 * capacity < n_entries. */
int simmr_ovleval_emit(simmr_ovleval* h, uint64_t* key_a_dev, uint64_t* key_b_dev, uint64_t* ov_dev, uint32_t* best_dev, uint32_t* hits_dev,
                       uint64_t capacity);
/* HIP-event time (ms) of the device work since the last reset: the truth adds, the plans and the adds.  Synchronises the stream.
 * A run of adds with no synchronising call of this object between them (the plan or this call) is timed as one span,
 * from the first add's start to the last one's end on the stream. */
int simmr_last_ovleval_ms(simmr_ovleval* h, float* ms);

/* ---- a variant caller's VCF scored against the strain's sites: two texts in HBM, joined and classified on the device ----------
 * Replaces nothing in the reference.  The third truth a run writes is the strain's sites (simmr_pileup_*, `--strain-vcf`): every
 * substituted position with the allele counts the run's reads show there.  The truth (that VCF, or any VCF that follows the
 * rules below) and a variant caller's VCF for the same reads go in, and integer tables come out: the calls correct and wrong and
 * why, by QUAL; the sites found, missed and called more than once; and found / not found by the number of reads that showed the
 * alternate base, which only the simulator knows.  No simulation, no genome: like simmr_mapeval_*.
 *
 * Text.  Whole lines of plain VCF (no gzip, no BCF): every line ends in '\n', except that the last line of a call may lack it;
 * the caller cuts a file at line ends, at most SIMMR_FIT_SAM_MAX_BYTES a call.  An empty line is skipped and not counted.  A line
 * that starts with '#' is a header line, counted and skipped.  Every other line is a record.
 *
 * Record.  At least 8 tab-separated fields: 1 CHROM, 2 POS, 3 ID, 4 REF, 5 ALT, 6 QUAL, 7 FILTER, 8 INFO.  Field 9 (FORMAT) and
 * field 10 (the first sample) are read if present; further samples are not read.
 * Malformed (sticky; simmr_vcfeval_read answers SIMMR_EINVAL, simmr_vcfeval_truth_plan too for the truth), checked on every
 * record of either side before any filter: fewer than 8 fields; a POS that is not a decimal number of 1 to 18 digits, is 0 or is
 * above 2^40; an empty REF or a REF with a byte outside ACGTNacgtn; an empty ALT; a QUAL that is neither "." nor
 * [0-9]+(\.[0-9]*)?([eE][+-]?[0-9]{1,3})? with at most 18 digits before the point.
 *
 * Names and key.  The caller hands in the contig names once (simmr_vcfeval_config), under the rule and the limits of
 * simmr_mapeval_reset; the library keeps them sorted in a device blob and resolves a CHROM by exact byte comparison.  The row of a
 * name is its place in that order.  key = row << 40 | (POS - 1): rows are below 2^24, positions below 2^40.
 *
 * Truth record.  REF and ALT are one base each of ACGT (either case, folded to upper) and differ; CHROM is among the names;
 * anything else is malformed on this side.  The entry holds the key, the ref class and the alt class (A C G T = 0 1 2 3) and
 * ad_alt: the second number of the first ';'-separated item of INFO whose text starts with "AD=", which must be
 * "AD=<r>,<a>" with r and a of 1 to 10 digits and a below 2^32 (anything else in that item is malformed); 0 where INFO has no
 * such item.  Two entries with one key: simmr_vcfeval_truth_plan answers SIMMR_EINVAL.  FILTER and the sample columns are not
 * read on this side.
 *
 * Candidate record, in this order (records counts every well-formed one):
 *   1. Filtered.  FILTER is neither "." nor "PASS" and use_filtered is 0: counted filtered, and the record is left out.
 *   2. The QUAL row.  qrow = min(255, floor(QUAL)), from the digits in integers: with n digits before the point and the exponent
 *      e, the floor is the number that the first n + e digits spell — the digits before the point, then those behind it, then
 *      zeros (none where n + e <= 0: row 0).  So a negative exponent shifts the point left and a positive one right through the
 *      fraction digits; a value whose integer part passes three digits is row 255.  "." is row 0, and the record is also counted
 *      qual_missing.
 *   3. The called alleles.  ALT is a comma-separated list of n_alt alleles.  If the record has a FORMAT that is "GT" or starts
 *      with "GT:" and a sample column, GT is the sample's text up to its first ':': items separated by '/' or '|', each "." or
 *      a decimal number of 1 to 18 digits (any other item is malformed, and so is a number above n_alt).  The called alleles are
 *      the ALT alleles whose 1-based index is among the numbers; a GT without a number of 1 or more is counted ref_call and the
 *      record is left out.  Without such a FORMAT or without a sample column every ALT allele is called.
 *   4. Each called allele, in ALT order, is one of:
 *        "*", or an allele that starts with '<' or contains '[' or ']': counted symbolic, no call;
 *        else a length other than REF's, or a byte outside ACGTNacgtn: counted indel, no call (the strain has substitutions
 *          only: these are counted and never scored as right or wrong);
 *        else a length L above 64: counted long_allele, no call;
 *        else one CALL at every offset j < L where the upper-cased ALT byte differs from the upper-cased REF byte and both are
 *          of ACGT: position POS + j, ref base REF[j], alt base ALT[j] (an SNV is L = 1, an MNP gives a call per changed base).
 *          An allele whose upper-cased bytes all equal REF's is counted ref_call_allele.
 *   5. A call's verdict (calls counts every call):
 *        CHROM is not among the names: unknown_contig, wrong.
 *        Else no entry has the key row << 40 | (POS + j - 1) (none can where POS + j - 1 reaches 2^40): no_site, wrong.
 *        Else the call's ref class differs from the entry's: ref_mismatch, wrong, class 2.
 *        Else the alt class differs: wrong_allele, wrong, class 2.                Else: correct, class 3.
 *      by_qual[qrow][class 3 ? 0 : 1] counts every call, the first two kinds under wrong.  The last three verdicts give the
 *      entry a hit: hits[entry] += 1, best[entry] = max(best[entry], class << 8 | qrow).
 *   6. wrong = unknown_contig + no_site + ref_mismatch + wrong_allele, and calls = wrong + correct.
 * Per truth entry, made by a reduction in simmr_vcfeval_read: sites_found (best's class is 3), sites_wrong (class 2),
 * sites_missed (no hit), sites_multiple (hits > 1), and by_ad[SIMMR_VCFEVAL_AD_ROWS][2]: the entries by the bit length of ad_alt
 * (0 for 0), [0] found and [1] not found — recall against the number of reads that showed the allele.
 * The truth is haploid: a called allele is a call whatever its zygosity.
 * Every output is an integer sum or maximum: the same for any launch geometry and any cut of either text into adds. */
#define SIMMR_VCFEVAL_AD_ROWS 33u   /* by_ad: row b holds the entries whose ad_alt has bit length b (ad_alt < 2^32) */

typedef struct simmr_vcfeval simmr_vcfeval;

typedef struct simmr_vcfeval_config {   /* HOST memory */
  uint32_t n_names;
  uint32_t use_filtered;                /* 0: a record whose FILTER is neither "." nor "PASS" is left out; else: it is scored */
  const char* const* rname;             /* n_names contig names, NUL-terminated, in any order */
} simmr_vcfeval_config;

typedef struct simmr_vcfeval_counts {   /* HOST; every entry an integer sum, in this order */
  uint64_t truth_lines, truth_header, truth_entries;   /* lines = header + records; cumulative since the reset */
  uint64_t lines, header, records;                     /* the candidate side, since the last truth plan */
  uint64_t filtered, qual_missing, ref_call;           /* records */
  uint64_t symbolic, indel, long_allele, ref_call_allele;   /* called alleles that give no call */
  uint64_t calls, unknown_contig, no_site, ref_mismatch, wrong_allele, correct, wrong;
  uint64_t sites_found, sites_wrong, sites_missed, sites_multiple;   /* truth entries: best class 3, class 2, no hit, more than one hit */
} simmr_vcfeval_counts;

/* The state is an object of its own, created on an engine and destroyed BEFORE the engine (as simmr_mapeval_create); its calls
 * run on the engine's stream and leave their messages with the engine (simmr_last_error). */
int simmr_vcfeval_create(simmr_engine* e, simmr_vcfeval** out);
void simmr_vcfeval_destroy(simmr_vcfeval* h);
/* Takes the names and use_filtered, and empties both sides.  Synchronises.  SIMMR_EINVAL: a NULL argument, a name given twice.
 * SIMMR_ENOTSUP: a name that is empty, longer than 254 bytes or no SAM reference name.  SIMMR_ERANGE: more than 2^24 names. */
int simmr_vcfeval_reset(simmr_vcfeval* h, const simmr_vcfeval_config* cfg);
/* Adds the records of text[0 .. n_bytes) (DEVICE memory, which must stay as it is until the stream has run the add) to the
 * truth.  Only enqueues.  Drops a truth plan.  Room for an entry per 15 bytes of text (no record is shorter: 8 one-byte fields
 * and 7 tabs) grows with the object.  SIMMR_ESTATE: no reset yet.  SIMMR_EINVAL: a NULL text with n_bytes > 0.  SIMMR_ENOTSUP:
 * n_bytes above SIMMR_FIT_SAM_MAX_BYTES. */
int simmr_vcfeval_truth_add(simmr_vcfeval* h, const uint8_t* text, uint64_t n_bytes);
/* Sorts the entries by key (the radix sort of simmr_sam_sort_plan, over the bits of the largest key), checks that no key stands
 * twice, empties the candidate side and synchronises.  *n_entries (may be NULL) = the entries.  SIMMR_EINVAL: a malformed truth
 * record, or two entries with one key.  SIMMR_ERANGE: 2^31 entries or more. */
int simmr_vcfeval_truth_plan(simmr_vcfeval* h, uint64_t* n_entries);
/* Scores the records of text[0 .. n_bytes) (DEVICE, as above) against the plan.  Only enqueues.  SIMMR_ESTATE: no truth plan
 * in force.  SIMMR_EINVAL, SIMMR_ENOTSUP: as simmr_vcfeval_truth_add. */
int simmr_vcfeval_add(simmr_vcfeval* h, const uint8_t* text, uint64_t n_bytes);
/* The counts, by_qual_host[256][2] (the calls by QUAL row, [0] correct and [1] wrong) and by_ad_host[SIMMR_VCFEVAL_AD_ROWS][2]
 * (HOST, any may be NULL).  Synchronises.  The sites_* counts and by_ad are made here, by a reduction over best[], hits[] and
 * ad[].  SIMMR_EINVAL: a malformed record on either side since the reset (nothing is written).  SIMMR_ESTATE: no reset yet. */
int simmr_vcfeval_read(simmr_vcfeval* h, simmr_vcfeval_counts* counts, uint64_t* by_qual_host, uint64_t* by_ad_host);
/* The truth entries in ascending key order (unique keys: the order is a function of the input), five columns (DEVICE, capacity
 * entries each, any may be NULL): key, alleles = ref class << 2 | alt class, ad = ad_alt, best = the maximum over the entry's
 * hits of class << 8 | qrow (0: no hit), hits.  Synchronises.  SIMMR_ESTATE: no truth plan.  SIMMR_ERANGE, nothing written:
 * capacity < n_entries. */
int simmr_vcfeval_emit(simmr_vcfeval* h, uint64_t* key_dev, uint32_t* alleles_dev, uint32_t* ad_dev, uint32_t* best_dev, uint32_t* hits_dev,
                       uint64_t capacity);
/* HIP-event time (ms) of the device work since the last reset: the truth adds, the plans and the adds.  Synchronises the stream.
 * A run of adds with no synchronising call of this object between them (the plan or this call) is timed as one span. */
int simmr_last_vcfeval_ms(simmr_vcfeval* h, float* ms);

/* ---- a read classifier's calls scored against each read's true genome: a taxonomy and two texts in HBM ------------------------
 * Replaces nothing in the reference.  A run over many genomes is a metagenome, and the fourth truth it writes is the one a
 * taxonomic read classifier is held against: `--truth` names the genome of every read.  That TSV, the per-read output of a
 * classifier (the format of Kraken 2, which Centrifuge and others can write), a taxonomy and the taxid of every genome go in, and
 * integer tables come out: per rank the records and the reads correct, right but less specific, wrong and unclassified, and per
 * taxon the reads that belong to it, that were called into it, and both.  No simulation, no genome: like simmr_mapeval_*.
 *
 * Taxonomy (simmr_taxeval_config, HOST arrays, taken by simmr_taxeval_reset).  n_nodes nodes: taxid[], parent[] (the parent's
 * taxid) and rank[].  Taxid 0 is reserved for "unclassified" and is no node.  A root is a node whose parent is itself or 0; there
 * may be several.  Rank codes: 1 domain (also "superkingdom"), 2 phylum, 3 class, 4 order, 5 family, 6 genus, 7 species, 8 strain;
 * 0 any other rank or none.  The reset sorts the nodes by taxid on the device; the ROW of a node is its place in that order.  It
 * resolves every parent to a row and builds, per node, its depth (the steps to its root; a root has depth 0) and the row of its
 * ancestor-or-self at each of the 8 ranks: the nearest node of that rank walking up from the node, itself included; none where
 * the lineage has no node of that rank.  SIMMR_EINVAL: a taxid of 0, a taxid given twice, a parent that is no node, a walk that
 * reaches no root within SIMMR_TAXEVAL_MAX_DEPTH steps (a cycle, or a tree deeper than that), a rank code above 8, a lineage that
 * holds one rank twice, a genome whose taxid is 0 or no node.  SIMMR_ERANGE: more than 2^26 nodes.
 * Genomes.  n_genomes pairs of genome_id[] (NUL-terminated, 1 to 254 bytes, no tab and no newline: SIMMR_ENOTSUP otherwise) and
 * genome_taxid[].  An id given twice is SIMMR_EINVAL, more than 2^24 of them SIMMR_ERANGE.  The library keeps the ids sorted
 * bytewise in a device blob and resolves a genome_id field by exact byte comparison; the genome ROW is the place in that order.
 *
 * Text, both sides.  Whole lines of plain text (no gzip): every line ends in '\n', except that the last line of a call may lack
 * it; the caller cuts a file at line ends, at most SIMMR_FIT_SAM_MAX_BYTES a call.  An empty line is skipped and not counted.  A
 * line whose first byte is '#', or that starts with "read_id<tab>", is a header line, counted and skipped.  Every other line is a
 * record.  Only the first three tab-separated fields of a record are read.
 *
 * Truth record: read_id, pair, genome_id.  Malformed (sticky; simmr_taxeval_truth_plan and simmr_taxeval_read answer SIMMR_EINVAL):
 * fewer than 3 fields; a read_id that is not 1 to 18 digits; a pair that is not exactly "0", "1" or "2"; a genome_id that is not
 * among the genomes.  The plan sorts the lines by read id and collapses equal ids into one ENTRY (id, genome row, mates = the
 * lines behind it: both mates of a pair come from one genome).  One id with two different genomes, or with more than two lines:
 * the plan answers SIMMR_EINVAL.
 *
 * Candidate record: "C" or "U", the read name, the taxon.  Malformed (sticky; simmr_taxeval_read answers SIMMR_EINVAL), checked
 * on every record before any step: fewer than 3 fields; a field 1 that is not exactly "C" or "U"; a field 3 that is neither 1 to
 * 10 digits with a value below 2^32 nor any text that ends in "(taxid <1 to 10 digits, below 2^32>)" (the --use-names form).
 * The read name is a read id of 1 to 18 digits with an optional "/1" or "/2" (the name rule of simmr_ovleval_*); the suffix is
 * dropped.  A record is handled in this order (records counts every well-formed one):
 *   1. A name that is no read id, or an id with no entry: unknown_read; not scored, no table changes.
 *   2. "U", or taxid 0: unclassified.  Class 1 at every rank the truth has, class 0 at the others.
 *   3. A taxid that is no node: unknown_taxon.  Class 2 at every rank the truth has, class 0 at the others.
 *   4. Otherwise scored.  With t = the node of the entry's genome and c = the called node, rank r = 1 .. 8 gets the class
 *        0 absent:   t has no ancestor-or-self at r;
 *        4 correct:  c has one, and it is the same row as t's;
 *        2 wrong:    c has one, and it is another row;
 *        3 above:    c has none, and c is an ancestor-or-self of t (the lowest common ancestor of t and c is c): right, but
 *                    less specific than r;
 *        2 wrong:    c has none, and c is not on t's path.
 * Every record of steps 2 to 4 updates: by_rank[r - 1][class] += 1 for each rank (class 0 included); hits[entry] += 1;
 * seen[entry] |= one bit per rank, bit 4 (r - 1) + class - 1 (class 0 sets none), so the best class of a read at rank r is the
 * highest set bit of nibble r - 1, plus one; and the direct per-node counts: n_true[t] += 1, and for step 4 also n_called[c] += 1
 * and n_both[lca(t, c)] += 1 (nothing where t and c stand under different roots).
 * Per entry, made by a reduction in simmr_taxeval_read: truth_paired (mates == 2), missing (no hit), multiple (more hits than
 * mates), and reads_by_rank[r - 1][class]: the entries by the best class of their records at r; an entry with no record counts as
 * class 1 at the ranks its genome has and 0 at the others.
 * Every output is an integer sum or an OR: the same for any launch geometry and any cut of either text into adds. */
#define SIMMR_TAXEVAL_RANKS 8u
#define SIMMR_TAXEVAL_CLASSES 5u        /* 0 absent, 1 unclassified, 2 wrong, 3 above, 4 correct */
#define SIMMR_TAXEVAL_MAX_DEPTH 255u    /* the longest walk from a node to its root, in steps */

typedef struct simmr_taxeval simmr_taxeval;

typedef struct simmr_taxeval_config {   /* HOST memory; every array in any order */
  uint64_t n_nodes;
  const uint32_t* taxid;                /* [n_nodes] */
  const uint32_t* parent;               /* [n_nodes] the parent's taxid; itself or 0: a root */
  const uint8_t* rank;                  /* [n_nodes] the rank code, 0 .. 8 */
  uint64_t n_genomes;
  const char* const* genome_id;         /* [n_genomes] NUL-terminated */
  const uint32_t* genome_taxid;         /* [n_genomes] */
} simmr_taxeval_config;

typedef struct simmr_taxeval_counts {   /* HOST; every entry an integer sum, in this order */
  uint64_t truth_lines, truth_header;                  /* lines = header + records; cumulative since the reset */
  uint64_t truth_entries, truth_paired;                /* of the plan in force: the entries, and those with two lines */
  uint64_t lines, header, records;                     /* the candidate side, since the last truth plan */
  uint64_t unknown_read, unclassified, unknown_taxon, scored;   /* records = the sum of these four */
  uint64_t missing, multiple;                          /* truth entries: no hit, more hits than lines */
} simmr_taxeval_counts;

/* The state is an object of its own, created on an engine and destroyed BEFORE the engine (as simmr_mapeval_create); its calls
 * run on the engine's stream and leave their messages with the engine (simmr_last_error). */
int simmr_taxeval_create(simmr_engine* e, simmr_taxeval** out);
void simmr_taxeval_destroy(simmr_taxeval* h);
/* Takes the taxonomy and the genomes, builds the tree on the device and empties both sides.  Synchronises.  The errors are those
 * of the two paragraphs above, and SIMMR_EINVAL for a NULL argument.  A reset that fails leaves the object without a tree: every
 * other call answers SIMMR_ESTATE until a reset succeeds. */
int simmr_taxeval_reset(simmr_taxeval* h, const simmr_taxeval_config* cfg);
/* The lineage of the node `taxid`: out_taxid[r - 1] (HOST, 8 words, may be NULL) = the taxid of its ancestor-or-self at rank r, 0
 * where it has none; *depth (may be NULL) = its steps to the root.  Synchronises.  SIMMR_EINVAL: no such node.  SIMMR_ESTATE. */
int simmr_taxeval_lineage(simmr_taxeval* h, uint32_t taxid, uint32_t* out_taxid, uint32_t* depth);
/* Adds the records of text[0 .. n_bytes) (DEVICE memory, which must stay as it is until the stream has run the add) to the
 * truth.  Only enqueues.  Drops a truth plan.  Room for a line per 5 bytes of text (no record is shorter: 3 one-byte fields and
 * 2 tabs) grows with the object.  SIMMR_ESTATE: no reset yet.  SIMMR_EINVAL: a NULL text with n_bytes > 0.  SIMMR_ENOTSUP:
 * n_bytes above SIMMR_FIT_SAM_MAX_BYTES. */
int simmr_taxeval_truth_add(simmr_taxeval* h, const uint8_t* text, uint64_t n_bytes);
/* Sorts the lines by read id (the radix sort of simmr_sam_sort_plan, over the bits of the largest id), collapses equal ids into
 * entries with a head flag, a scan and a compaction, empties the candidate side and synchronises.  *n_entries (may be NULL) = the
 * entries.  SIMMR_EINVAL: a malformed truth record, one id with two genomes or with more than two lines.  SIMMR_ERANGE: 2^31
 * lines or more. */
int simmr_taxeval_truth_plan(simmr_taxeval* h, uint64_t* n_entries);
/* Scores the records of text[0 .. n_bytes) (DEVICE, as above) against the plan.  Only enqueues.  SIMMR_ESTATE: no truth plan
 * in force.  SIMMR_EINVAL, SIMMR_ENOTSUP: as simmr_taxeval_truth_add. */
int simmr_taxeval_add(simmr_taxeval* h, const uint8_t* text, uint64_t n_bytes);
/* The counts, by_rank_host[8][5] (the records by rank and class) and reads_by_rank_host[8][5] (the entries by rank and best
 * class) (HOST, any may be NULL).  Synchronises.  truth_paired, missing, multiple and reads_by_rank are made here, by a reduction
 * over seen[], hits[] and mates[].  SIMMR_EINVAL: a malformed record on either side since the reset (nothing is written).
 * SIMMR_ESTATE: no reset yet. */
int simmr_taxeval_read(simmr_taxeval* h, simmr_taxeval_counts* counts, uint64_t* by_rank_host, uint64_t* reads_by_rank_host);
/* The truth entries in ascending id order, five columns (DEVICE, capacity entries each, any may be NULL): the read id, the genome
 * row, mates (the lines behind the entry, 1 or 2), seen and hits.  Synchronises.  SIMMR_ESTATE: no truth plan.  SIMMR_ERANGE,
 * nothing written: capacity < n_entries. */
int simmr_taxeval_emit(simmr_taxeval* h, uint64_t* id_dev, uint32_t* genome_row_dev, uint32_t* mates_dev, uint32_t* seen_dev, uint32_t* hits_dev,
                       uint64_t capacity);
/* One row per node in taxid order, four columns (DEVICE, capacity_nodes each, any may be NULL): the taxid and the three CLADE sums
 * — a node's sum over itself and all its descendants of n_true, n_called and n_both.  So for a node X of rank r, called[X] counts
 * the records called into X at r or below, true[X] those that truly belong to it, and both[X] the true positives.  The direct
 * counts are only read: the sums are made anew by every call, and a second call gives the same answer.  Synchronises.
 * SIMMR_ESTATE: no reset yet.  SIMMR_ERANGE, nothing written: capacity_nodes < n_nodes. */
int simmr_taxeval_taxa(simmr_taxeval* h, uint32_t* taxid_dev, uint64_t* true_dev, uint64_t* called_dev, uint64_t* both_dev, uint64_t capacity_nodes);
/* HIP-event time (ms) of the device work since the last reset: the truth adds, the plans and the adds (not the reset's tree).
 * Synchronises the stream.  A run of adds with no synchronising call of this object between them is timed as one span. */
int simmr_last_taxeval_ms(simmr_taxeval* h, float* ms);

/* ---- an assembler's contigs scored against the gold-standard assembly: two FASTA texts in HBM, compared by canonical k-mers -----
 * Replaces nothing in the reference.  The fifth truth a run writes is the gold-standard assembly (simmr_regions_*,
 * `--gold-assembly`): the stretches of every genome that the reads covered.  That FASTA and an assembler's contigs go in, and
 * integer tables come out, alignment-free: how many of each genome's distinct k-mers the contigs hold (completeness), how many of
 * the contigs' k-mers are in no genome (the consensus quality), and for every contig the genome most of its k-mers vote for.  No
 * simulation, no genome: like simmr_mapeval_*.
 *
 * Text.  Plain FASTA (no gzip).  One add holds whole records: its first non-empty line starts with '>', and the caller cuts a
 * file in front of a '>' that begins a line, at most SIMMR_ASMEVAL_MAX_BYTES a call.  A line that starts with '>' is a header;
 * every other non-empty line is a sequence line of the record above it.  Empty lines are skipped.  A '\r' directly before '\n'
 * is not a base (a line that holds nothing else is empty); the last line may lack its '\n', and then a '\r' that ends it is a
 * byte like any other.  A '>' that does not begin a line is an ordinary byte of the line it stands in.
 * Malformed (sticky; simmr_asmeval_read answers SIMMR_EINVAL, simmr_asmeval_truth_plan too for the truth): a sequence line with a
 * base in front of the add's first header.
 *
 * Bases and k-mers.  Every byte of a sequence line is one base position, apart from the line end.  ACGTacgt are the classes
 * 0 1 2 3 with case folded; any other byte is an invalid base.  k is odd and lies between 15 and 31, so no k-mer is its own
 * reverse complement.  A k-mer is k consecutive valid bases of one record; line ends are transparent to it, and a record shorter
 * than k has none.  Its first base is the most significant digit of its 2k-bit value, and its key is the smaller of that value
 * and the value of its reverse complement.
 *
 * Truth side.  The genome of a truth record is the header's text between '>' and the first '|' of its first word (the word ends
 * at a blank, a tab or the line's end): `--gold-assembly` writes ">GENOME|SEQ:start-end depth_sum=N".  The caller hands in the
 * genome names once (simmr_asmeval_config), under the rule and the limits of simmr_mapeval_reset, fewer than 2^24 of them; the
 * library keeps them sorted in a device blob and compares bytes exactly.  The row of a genome is its place in that order.  A
 * header with no '|' in its first word, or with a prefix that is not among the names, is malformed.  simmr_asmeval_truth_add
 * appends every k-mer occurrence as (key, genome row).  simmr_asmeval_truth_plan (1) sorts the occurrences by key over 2k bits,
 * (2) marks the run heads and scans them, (3) compacts the runs into the distinct entries in ascending key order, builds the
 * lookup table (min(24, bit length of the entries) of the key's top bits) and (4) empties the candidate side and synchronises.
 * An entry has key, mult (its occurrences) and genome: the one row all its occurrences share, or the row n_genomes ("shared")
 * where they come from two genomes or more.
 *
 * Candidate side.  A contig is a record; its row is its ordinal among the candidate records since the truth plan, in add order
 * and then text order.  Candidate headers are not read beyond their extent.  Every k-mer of a contig is looked up among the
 * entries: a miss is novel; a hit is found and hits[entry] += 1 (hits is below 2^32); a hit on a shared entry is also shared; a
 * hit on an entry of one genome is a vote of the contig for that genome.  top_genome is the genome with the most votes (ties go
 * to the lowest row) and top_kmers its votes; without a vote they are 0xffffffff and 0.  Six columns per contig: length in
 * bases (u64, invalid ones included), kmers, found, shared, top_genome, top_kmers (u32).
 *
 * Tables (simmr_asmeval_read).  The counts below; the contig classes are exclusive and their sum is records: contigs_short (no
 * k-mer), contigs_novel (k-mers, none found), contigs_pure (votes, all for one genome), contigs_mixed (votes for two genomes or
 * more), contigs_shared_only (found k-mers, no vote).  by_genome[n_genomes + 1][SIMMR_ASMEVAL_GENOME_COLS], the last row
 * "shared": distinct (the entries of that row), distinct_found (those with a hit), over (those whose hits exceed mult: the
 * assembly holds the k-mer more often than the truth), contigs (whose top_genome is the row) and contig_bases (their lengths);
 * the shared row has 0 in the last two.
 * Every output is an integer sum or maximum: the same for any launch geometry, for any cut of either text into adds, and when
 * any candidate record is replaced by its reverse complement. */
#define SIMMR_ASMEVAL_MAX_BYTES 0x7fffffffull   /* most bytes of text in one add of either side */
#define SIMMR_ASMEVAL_GENOME_COLS 5u            /* by_genome: distinct, distinct_found, over, contigs, contig_bases */

typedef struct simmr_asmeval simmr_asmeval;

typedef struct simmr_asmeval_config {   /* HOST memory */
  uint32_t n_genomes;
  uint32_t k;                           /* odd, 15 .. 31 */
  uint32_t plain_search;                /* 0: a lookup goes through the table of the key's top bits; else: a binary search over all entries (the same answers) */
  const char* const* genome;            /* n_genomes genome names, NUL-terminated, in any order */
} simmr_asmeval_config;

typedef struct simmr_asmeval_counts {   /* HOST; every entry an integer sum, in this order */
  uint64_t truth_records, truth_bases, truth_invalid, truth_kmers;   /* cumulative since the reset; kmers = occurrences */
  uint64_t truth_distinct, truth_shared_distinct;                    /* the entries of the plan in force, and those of two genomes or more */
  uint64_t records, bases, invalid, kmers, found, shared, novel;     /* the candidate side, since the last truth plan; novel = kmers - found */
  uint64_t contigs_short, contigs_novel, contigs_pure, contigs_mixed, contigs_shared_only;
} simmr_asmeval_counts;

/* The state is an object of its own, created on an engine and destroyed BEFORE the engine (as simmr_vcfeval_create); its calls
 * run on the engine's stream and leave their messages with the engine (simmr_last_error). */
int simmr_asmeval_create(simmr_engine* e, simmr_asmeval** out);
void simmr_asmeval_destroy(simmr_asmeval* h);
/* Takes the names, k and the lookup, and empties both sides.  Synchronises.  SIMMR_EINVAL: a NULL argument, a name given twice, a
 * k that is even, below 15 or above 31.  SIMMR_ENOTSUP: a name that is empty, longer than 254 bytes or no SAM reference name.
 * SIMMR_ERANGE: 2^24 names or more. */
int simmr_asmeval_reset(simmr_asmeval* h, const simmr_asmeval_config* cfg);
/* Adds the records of text[0 .. n_bytes) (DEVICE memory, which must stay as it is until the stream has run the add) to the
 * truth.  Only enqueues.  Drops a truth plan.  Room for a k-mer occurrence per byte of text grows with the object.
 * SIMMR_ESTATE: no reset yet.  SIMMR_EINVAL: a NULL text with n_bytes > 0.  SIMMR_ENOTSUP: n_bytes above SIMMR_ASMEVAL_MAX_BYTES. */
int simmr_asmeval_truth_add(simmr_asmeval* h, const uint8_t* text, uint64_t n_bytes);
/* The plan, in the order stated above.  Synchronises.  *n_entries (may be NULL) = the distinct entries.  SIMMR_EINVAL: a malformed
 * truth text.  SIMMR_ERANGE: 2^31 k-mer occurrences or more since the reset. */
int simmr_asmeval_truth_plan(simmr_asmeval* h, uint64_t* n_entries);
/* Scores the records of text[0 .. n_bytes) (DEVICE, as above) against the plan.  SYNCHRONISES, three times: it needs the add's
 * records and bases on the host for the contig columns, and the number of its votes for their sort and scan.  SIMMR_ESTATE: no
 * truth plan in force.  SIMMR_ERANGE: 2^31 contigs or more since the plan.  SIMMR_EINVAL, SIMMR_ENOTSUP: as
 * simmr_asmeval_truth_add. */
int simmr_asmeval_add(simmr_asmeval* h, const uint8_t* text, uint64_t n_bytes);
/* The counts and by_genome_host[n_genomes + 1][SIMMR_ASMEVAL_GENOME_COLS] (HOST, either may be NULL).  Synchronises.  The
 * candidate counts, the contig classes and by_genome are made here, by reductions over the entry and contig columns that combine
 * the first 1024 rows in LDS.  SIMMR_EINVAL: a malformed text on either side since the reset (nothing is written).
 * SIMMR_ESTATE: no reset yet. */
int simmr_asmeval_read(simmr_asmeval* h, simmr_asmeval_counts* counts, uint64_t* by_genome_host);
/* The entries in ascending key order, four columns (DEVICE, capacity entries each, any may be NULL): key, genome, mult, hits.
 * Synchronises.  SIMMR_ESTATE: no truth plan.  SIMMR_ERANGE, nothing written: capacity < n_entries. */
int simmr_asmeval_emit(simmr_asmeval* h, uint64_t* key_dev, uint32_t* genome_dev, uint32_t* mult_dev, uint32_t* hits_dev, uint64_t capacity);
/* The contigs in row order, six columns (DEVICE, capacity entries each, any may be NULL).  *n_contigs (may be NULL) = the contigs
 * since the plan, written whenever a plan is in force: a call with capacity 0 asks for it.  Synchronises.  SIMMR_ESTATE: no truth
 * plan.  SIMMR_ERANGE, no column written: capacity < the contigs. */
int simmr_asmeval_contigs(simmr_asmeval* h, uint64_t* length_dev, uint32_t* kmers_dev, uint32_t* found_dev, uint32_t* shared_dev, uint32_t* top_genome_dev,
                          uint32_t* top_kmers_dev, uint64_t capacity, uint64_t* n_contigs);
/* HIP-event time (ms) of the device work since the last reset: the truth adds, the plans and the adds.  Synchronises the stream.
 * A run of adds with no synchronising call of this object between them (the plan or this call) is timed as one span; the host's
 * waits inside simmr_asmeval_add lie inside that span.  *plan_sort_ms (may be NULL) = the sort's share of the last plan. */
int simmr_last_asmeval_ms(simmr_asmeval* h, float* ms, float* plan_sort_ms);

/* ---- an assembler's contigs PLACED on the gold-standard assembly: anchors, collinear blocks and the breakpoints between them -----
 * Replaces nothing in the reference.  simmr_asmeval_* is alignment-free and cannot tell a correct contig from a chimera of two
 * genomes; this object gives every k-mer of the truth its POSITION, so that a contig falls into collinear blocks on the truth
 * records and the places where the blocks change are the misassemblies (metaQUAST's classes, and the blocks NA50 / NGA50 are
 * computed from).  All of it is integer arithmetic.  No simulation, no genome: like simmr_asmeval_*.
 *
 * Text, bases, k-mers, keys, genome names, malformed texts: the rules of simmr_asmeval_* above, word for word, with
 * SIMMR_ASMEVAL_MAX_BYTES a call.
 *
 * Truth side.  A truth record's row t is its ordinal among the truth records since the reset, in add order and then text order;
 * its genome row is as in asmeval.  Every k-mer occurrence carries its key, t, p (the position of its first base in the record,
 * counting every base position, invalid ones included) and o (1 where the key is the reverse complement's value, else 0).
 * simmr_asmmap_truth_plan sorts the occurrences by key over 2k bits and keeps as ANCHORS the keys that occur exactly once in the
 * whole truth; a key with two occurrences or more, in one genome or several, anchors nothing: it is a REPEAT.  The anchor index is
 * (key, t, p, o) in ascending key order behind asmeval's prefix table (min(24, bit length of the entries) of the key's top
 * bits); the distinct repeat keys stand in a second index of the same kind, searched only where the first misses, so that a
 * repeat is told from a k-mer the truth does not hold.  The plan empties the candidate side and synchronises.
 *
 * Candidate side.  A contig's row c is defined as in asmeval.  A k-mer of a contig has its first base at q (in the record, as p)
 * and its orientation bit oc.  A hit on an anchor key is an ANCHOR HIT with relative strand s = oc ^ o and the diagonal d, a signed
 * 64-bit number: d = p - q where s = 0, d = p + q where s = 1.  The hits of an add are compacted in (contig, q) order by a count
 * pass, a scan and a write pass, never appended by atomics: their order is the data.
 * Runs.  In that order a hit starts a new run where it is the first hit of its contig, where its t or its s differs from the
 * previous hit's, or where |d - d_prev| > band.  A run with fewer than min_anchors hits is STRAY: it is dropped and its hits count
 * in stray_hits.
 * Blocks.  Over the kept runs of a contig, in order, a run starts a new block where it is the contig's first kept run, where its
 * t or s differs from the previous kept run's, or where |d_first - d_last of the previous kept run| > band.  That is ONE merge
 * round: a dropped run between two runs on one diagonal does not break them.  Nine columns a block: contig, truth_record, strand,
 * q_start (the first hit's q), q_end (the last hit's q + k), p_start (the smallest p), p_end (the largest p + k), hits, join.
 * Blocks stand in (contig, q) order.
 * Breakpoints.  join of a contig's first block is 0; of every further block it is the class of the step from the block before it,
 * the first that applies: SIMMR_ASMMAP_INTER_GENOME (the two truth records belong to different genomes), _INTER_RECORD (one genome,
 * another truth record; the gold assembly's records are covered regions, so this also marks a contig that bridges a coverage
 * gap), _INVERSION (one record, the other strand), _RELOCATION (one record and strand, |dd| > relocation), _LOCAL (one record and
 * strand, band < |dd| <= relocation); dd is taken between the last hit of the earlier block and the first hit of the later one.
 *
 * Tables (simmr_asmmap_read; every entry an integer sum or maximum).  The counts below.  truth_repeats are the distinct repeat
 * keys; repeat_hits the candidate k-mers that found one; block_bases the sum of q_end - q_start.  The contig classes are exclusive
 * and sum to records: contigs_unplaced (no block), contigs_clean (one block), contigs_local_only (two blocks or more, every join
 * local), contigs_misassembled (any other join); misassembled_bases are the lengths of the last.
 * by_genome[n_genomes][SIMMR_ASMMAP_GENOME_COLS]: truth_bases, truth_anchors, and by the genome of the block's truth record
 * blocks, block_bases, longest_block (a maximum).
 * Contig columns (simmr_asmmap_contigs): length (u64), hits, blocks, first_block (the row of its first block, 0xffffffff: none),
 * block_bases (u64), worst_join (the smallest non-zero join class among its blocks, 0: none).
 * Invariances.  Every count, by_genome, the contig columns other than first_block and the multiset of (contig, truth_record, hits,
 * q_end - q_start, p_start, p_end) of the blocks are the same for any launch geometry, for any cut of either text into adds at
 * record boundaries, and when any contig is replaced by its reverse complement: the run rule and the block rule are symmetric in
 * their two neighbours, and d only shifts by the constant L - k under the reversal of a contig of L bases.
 * Limits: a record shorter than 2^32 bases, fewer than 2^31 k-mer occurrences and fewer than 2^31 truth records (SIMMR_ERANGE). */
#define SIMMR_ASMMAP_GENOME_COLS 5u   /* by_genome: truth_bases, truth_anchors, blocks, block_bases, longest_block */
#define SIMMR_ASMMAP_BLOCK_COLS 9u    /* contig, truth_record, strand, q_start, q_end, p_start, p_end, hits, join */
#define SIMMR_ASMMAP_INTER_GENOME 1u
#define SIMMR_ASMMAP_INTER_RECORD 2u
#define SIMMR_ASMMAP_INVERSION 3u
#define SIMMR_ASMMAP_RELOCATION 4u
#define SIMMR_ASMMAP_LOCAL 5u

typedef struct simmr_asmmap simmr_asmmap;

typedef struct simmr_asmmap_config {   /* HOST memory */
  uint32_t n_genomes;
  uint32_t k;                          /* odd, 15 .. 31 */
  uint32_t band;                       /* two neighbours lie on one diagonal where their d differ by at most this (64 through Python and the CLI) */
  uint32_t relocation;                 /* a step of more than this is a relocation (1000: QUAST's extensive misassembly); below 2^31 */
  uint32_t min_anchors;                /* a run of fewer hits is stray (16); at least 1 */
  const char* const* genome;           /* n_genomes genome names, NUL-terminated, in any order */
} simmr_asmmap_config;

typedef struct simmr_asmmap_counts {   /* HOST; every entry an integer sum, in this order */
  uint64_t truth_records, truth_bases, truth_invalid, truth_kmers;   /* cumulative since the reset; kmers = occurrences */
  uint64_t truth_anchors, truth_repeats;                             /* of the plan in force */
  uint64_t records, bases, invalid, kmers, hits, stray_hits, repeat_hits;   /* the candidate side, since the last truth plan */
  uint64_t runs, runs_dropped, blocks, block_bases;
  uint64_t breaks_inter_genome, breaks_inter_record, breaks_inversion, breaks_relocation, breaks_local;
  uint64_t contigs_unplaced, contigs_clean, contigs_local_only, contigs_misassembled;
  uint64_t misassembled_bases;
} simmr_asmmap_counts;

/* The state is an object of its own, created on an engine and destroyed BEFORE the engine (as simmr_asmeval_create); its calls
 * run on the engine's stream and leave their messages with the engine (simmr_last_error).  simmr_asmmap_create reads the
 * environment variable SIMMR_ASMMAP_MAX_WGS once: a positive number caps the workgroups of every launch of the k_amap_* kernels of
 * this object (not of the text-to-planes stage it shares with asmeval).  It is there for tests and measurements of the launch
 * geometry; no answer depends on it. */
int simmr_asmmap_create(simmr_engine* e, simmr_asmmap** out);
void simmr_asmmap_destroy(simmr_asmmap* h);
/* Takes the names, k and the three thresholds, and empties both sides.  Synchronises.  SIMMR_EINVAL: a NULL argument, a name
 * given twice, a k that is even, below 15 or above 31, band above relocation, min_anchors of 0, relocation of 2^31 or more.
 * SIMMR_ENOTSUP, SIMMR_ERANGE for the names: as simmr_asmeval_reset. */
int simmr_asmmap_reset(simmr_asmmap* h, const simmr_asmmap_config* cfg);
/* Adds the records of text[0 .. n_bytes) (DEVICE memory, which must stay as it is until the stream has run the add) to the
 * truth.  Only enqueues.  Drops a truth plan.  Room for a k-mer occurrence per byte of text grows with the object.
 * SIMMR_ESTATE: no reset yet.  SIMMR_EINVAL: a NULL text with n_bytes > 0.  SIMMR_ENOTSUP: n_bytes above SIMMR_ASMEVAL_MAX_BYTES. */
int simmr_asmmap_truth_add(simmr_asmmap* h, const uint8_t* text, uint64_t n_bytes);
/* The plan, as stated above.  Synchronises.  *n_anchors (may be NULL) = the anchors.  SIMMR_EINVAL: a malformed truth text.
 * SIMMR_ERANGE: 2^31 k-mer occurrences or truth records or more since the reset. */
int simmr_asmmap_truth_plan(simmr_asmmap* h, uint64_t* n_anchors);
/* Places the records of text[0 .. n_bytes) (DEVICE, as above) on the plan.  SYNCHRONISES, five times: it needs the add's records
 * and bases on the host for the contig columns, and then the totals of four scans, each of which sizes what the next stage
 * writes: the anchor hits, the runs, the kept runs and the blocks.  SIMMR_ESTATE: no truth plan in force.  SIMMR_ERANGE: 2^31
 * contigs, or 2^32 - 1 blocks, or more since the plan.  SIMMR_EINVAL, SIMMR_ENOTSUP: as simmr_asmmap_truth_add. */
int simmr_asmmap_add(simmr_asmmap* h, const uint8_t* text, uint64_t n_bytes);
/* The counts and by_genome_host[n_genomes][SIMMR_ASMMAP_GENOME_COLS] (HOST, either may be NULL).  Synchronises.  The block and
 * contig sums are made here, by reductions over the block and contig columns.  Without a plan in force (none yet, or dropped by a
 * truth add) truth_anchors, truth_repeats, every candidate count and every column of by_genome are 0.  SIMMR_EINVAL: a malformed text on either side
 * since the reset (nothing is written).  SIMMR_ESTATE: no reset yet. */
int simmr_asmmap_read(simmr_asmmap* h, simmr_asmmap_counts* counts, uint64_t* by_genome_host);
/* The anchor index in ascending key order, four columns (DEVICE, capacity entries each, any may be NULL): key, t, p, o.
 * Synchronises.  SIMMR_ESTATE: no truth plan.  SIMMR_ERANGE, nothing written: capacity < the anchors. */
int simmr_asmmap_anchors(simmr_asmmap* h, uint64_t* key_dev, uint32_t* t_dev, uint32_t* p_dev, uint32_t* o_dev, uint64_t capacity);
/* The blocks in row order, SIMMR_ASMMAP_BLOCK_COLS columns in the order stated above (DEVICE; cols_dev is a HOST array of nine
 * device pointers of capacity entries each, any of which may be NULL, or NULL itself).  *n_blocks (may be NULL) = the blocks since
 * the plan, written whenever a plan is in force: a call with capacity 0 asks for it.  Synchronises.  SIMMR_ESTATE: no truth plan.
 * SIMMR_ERANGE, no column written: capacity < the blocks. */
int simmr_asmmap_blocks(simmr_asmmap* h, uint32_t* const* cols_dev, uint64_t capacity, uint64_t* n_blocks);
/* The contigs in row order, six columns (DEVICE, capacity entries each, any may be NULL); *n_contigs and the errors as
 * simmr_asmmap_blocks. */
int simmr_asmmap_contigs(simmr_asmmap* h, uint64_t* length_dev, uint32_t* hits_dev, uint32_t* blocks_dev, uint32_t* first_block_dev, uint64_t* block_bases_dev,
                         uint32_t* worst_join_dev, uint64_t capacity, uint64_t* n_contigs);
/* HIP-event time (ms) of the device work since the last reset: the truth adds, the plans and the adds.  Synchronises the stream.
 * A run of adds with no synchronising call of this object between them (the plan or this call) is timed as one span; the host's
 * waits inside simmr_asmmap_add lie inside that span. */
int simmr_last_asmmap_ms(simmr_asmmap* h, float* ms);

/* ---- a binner's contig bins scored against each contig's true genome: two tab-separated texts in HBM, joined by name -----------
 * Replaces nothing in the reference.  `--eval-assembly-contigs` writes, per contig, its name, its length and the genome most of
 * its k-mers vote for; a binner (MetaBAT, CONCOCT, MaxBin, VAMB, DAS Tool) puts the same contigs into bins.  Both texts go in and
 * integer tables come out: the (bin, genome) contingency table in contigs and in bases, every bin's purity and every genome's
 * completeness, the pair sums of the adjusted Rand index and CAMI's bin classes.  No simulation, no genome: like simmr_asmeval_*.
 *
 * Truth text.  Plain text (no gzip), eight tab-separated fields a line: field 1 the contig's name, field 2 its length in bases,
 * field 8 the genome's name, or "." for a contig without a top genome; fields 3 to 7 are only checked to be numbers.  A number is
 * one to eighteen decimal digits.  Further fields are ignored.  Empty lines are skipped, and so are lines that begin with '#'.  A
 * '\r' directly before '\n' is not part of the line (a line that holds nothing else is empty); the last line may lack its '\n',
 * and then a '\r' that ends it is a byte like any other.  The caller cuts a file behind a '\n', at most SIMMR_BINEVAL_MAX_BYTES a
 * call.
 * Names.  A contig name or a bin name is 1 to 254 bytes, none of them a tab, a blank or a control byte (0x00 .. 0x20, 0x7f).  Two
 * names are the same name exactly when their bytes are equal: nothing is trimmed, folded or parsed.  The genome names are handed in
 * once (simmr_bineval_config), under the rule and the limits of simmr_mapeval_reset, fewer than 2^24 of them; the row of a genome
 * is its place in the library's sorted order, and row n_genomes is "none" (".").
 * Candidate text.  A binner's assignment, one record a line: contig name, tab, bin name; further tab-separated fields are ignored.
 * Lines that begin with '#' or '@' are no records (the CAMI bioboxes head "@Version:", "@@SEQUENCEID BINID" passes unchanged);
 * line ends as in the truth.  A record's ordinal counts the records since the truth plan, in add order and then text order.
 * Malformed (sticky, the truth until the reset and the candidate until the next plan; simmr_bineval_truth_plan for the truth and
 * simmr_bineval_read for the candidate answer SIMMR_EINVAL and write nothing): a truth line with
 * fewer than eight fields, a field 2 to 7 that is no number, a genome name that is neither "." nor among the names, a contig name
 * that occurs twice in the truth, on either side an empty name or one longer than 254 bytes or with a byte a name may not hold, a
 * candidate record without a second field.
 *
 * The join.  The hash of a name is 64-bit FNV-1a over its bytes (SIMMR_BINEVAL_FNV_OFFSET, SIMMR_BINEVAL_FNV_PRIME).
 * simmr_bineval_truth_plan sorts the truth contigs by the low hash_bits bits of their hash; a lookup finds the run of equal
 * truncated hash by a binary search and walks it comparing bytes: the hash only narrows the search, byte equality decides.
 * hash_bits may be 0 to 64 (64 is what a caller without a reason gives); with 0 every name shares one run.  The answers are the
 * same for every value.  The object copies the names it needs (the truth's contig names, the records' bin names)
 * into buffers of its own: the caller's text may change once the stream has run the add.
 * Assignment.  A record whose contig is not in the truth is an unknown_contig: counted, not scored.  A truth contig named by
 * several records belongs to the bin of the record with the lowest ordinal; the others are `repeated`.  A truth contig named by no
 * record is unassigned.
 * Bins.  A bin is a distinct bin name among the records of known contigs, repeated ones included.  A bin's row is its rank by
 * first appearance, the lowest ordinal of a record of a known contig that carries the name (first_record).
 * The table.  A cell is (bin, genome row) with contigs and bases: the count and the summed lengths of the assigned truth contigs
 * of that bin whose true genome is that row, "none" included; cells are in (bin, genome) order.  Per bin: contigs, bases,
 * none_bases, first_record, and top_genome with top_bases: the real genome (never "none") with the most bases in the bin, ties to
 * the lowest row; without a real genome 0xffffffff and 0.  by_genome[n_genomes + 1][SIMMR_BINEVAL_GENOME_COLS]: truth_contigs,
 * truth_bases (assigned or not), assigned_contigs, assigned_bases, bins (the bins that hold any of it), best_bin and best_bases:
 * the bin with the most of the genome's bases, ties to the lowest bin row; without any 0xffffffff and 0.  The "none" row has 0 in
 * the last three.  A maximum is taken over the 64-bit bases alone and the lowest row that reaches it by a second pass, so no bits
 * go to a row: bins below 2^31 and any bases fit.  Base limit: the lengths of the truth sum to less than 2^57 (the classes
 * multiply a sum by 100); it is the caller's to keep.
 * Counts.  pairs_cells, pairs_bins and pairs_genomes are the sums of n (n - 1) / 2 over the cells', the bins' and the genome
 * rows' contig counts, over assigned contigs with a real genome.  The six classes are cumulative, as CAMI prints them: with t the
 * bin's top genome, a bin counts in bins_cC_xX where 100 * top_bases >= C * truth_bases[t] and 100 * (bases - top_bases) <= X *
 * bases, in integers.  A bin without a top genome is in none.  A contig in no genome is contamination: a bin's purity is
 * top_bases / bases, "none" bases included.
 * Every output is an integer sum, minimum or maximum: the same for any launch geometry, any cut of either text into adds at line
 * ends and any hash_bits; the same under any renaming of the bins that keeps them distinct, and under any reordering of the
 * candidate's lines that keeps the order of the bins' first appearances and, for every contig, which of its records comes first.
 * One engine. */
#define SIMMR_BINEVAL_MAX_BYTES 0x7fffffffull         /* most bytes of text in one add of either side */
#define SIMMR_BINEVAL_GENOME_COLS 7u                  /* by_genome: truth_contigs, truth_bases, assigned_contigs, assigned_bases, bins, best_bin, best_bases */
#define SIMMR_BINEVAL_FNV_OFFSET 0xcbf29ce484222325ull /* 64-bit FNV-1a: h = offset; for every byte: h = (h ^ byte) * prime */
#define SIMMR_BINEVAL_FNV_PRIME 0x100000001b3ull

typedef struct simmr_bineval simmr_bineval;

typedef struct simmr_bineval_config {   /* HOST memory */
  uint32_t n_genomes;
  uint32_t hash_bits;                   /* 0 .. 64: the low bits of the hash that order the truth and the records (64 unless a test wants long runs) */
  const char* const* genome;            /* n_genomes genome names, NUL-terminated, in any order */
} simmr_bineval_config;

typedef struct simmr_bineval_counts {   /* HOST; every entry an integer sum, in this order */
  uint64_t truth_records, truth_bases, truth_none;                        /* the truth of the plan in force; none: contigs whose genome is "." */
  uint64_t records, unknown_contig, repeated, assigned, assigned_bases;   /* the candidate side, since the last truth plan */
  uint64_t bins, cells;
  uint64_t sum_top_bases, sum_best_bases;                                 /* over the bins; over the real genomes */
  uint64_t pairs_cells, pairs_bins, pairs_genomes;
  uint64_t bins_c90_x5, bins_c70_x5, bins_c50_x5, bins_c90_x10, bins_c70_x10, bins_c50_x10;
} simmr_bineval_counts;

/* The state is an object of its own, created on an engine and destroyed BEFORE the engine (as simmr_asmeval_create); its calls
 * run on the engine's stream and leave their messages with the engine (simmr_last_error). */
int simmr_bineval_create(simmr_engine* e, simmr_bineval** out);
void simmr_bineval_destroy(simmr_bineval* h);
/* Takes the names and hash_bits, and empties both sides.  Synchronises.  SIMMR_EINVAL: a NULL argument, a name given twice, a
 * hash_bits above 64.  SIMMR_ENOTSUP: a name that is empty, longer than 254 bytes or no
 * SAM reference name.  SIMMR_ERANGE: 2^24 names or more. */
int simmr_bineval_reset(simmr_bineval* h, const simmr_bineval_config* cfg);
/* Adds the records of text[0 .. n_bytes) (DEVICE memory, which must stay as it is until the stream has run the add) to the
 * truth.  Only enqueues.  Drops a truth plan.  Room for a contig per 16 bytes of text and for the names grows with the object.
 * SIMMR_ESTATE: no reset yet.  SIMMR_EINVAL: a NULL text with n_bytes > 0.  SIMMR_ENOTSUP: n_bytes above SIMMR_BINEVAL_MAX_BYTES. */
int simmr_bineval_truth_add(simmr_bineval* h, const uint8_t* text, uint64_t n_bytes);
/* The plan: sorts the truth's contigs by the low hash_bits bits of their hash, looks for a name that occurs twice, and empties the
 * candidate side.  Synchronises.  *n_contigs (may be NULL) = the truth's contigs.  SIMMR_EINVAL: a malformed truth text.
 * SIMMR_ERANGE: 2^31 truth contigs or more since the reset. */
int simmr_bineval_truth_plan(simmr_bineval* h, uint64_t* n_contigs);
/* Joins the records of text[0 .. n_bytes) (DEVICE, as above) to the truth.  SYNCHRONISES, once: it needs the add's records and the
 * bytes of their bin names on the host, for the room of the record columns.  SIMMR_ESTATE: no truth plan in force.  SIMMR_ERANGE:
 * 2^31 records or more since the plan.  SIMMR_EINVAL, SIMMR_ENOTSUP: as simmr_bineval_truth_add. */
int simmr_bineval_add(simmr_bineval* h, const uint8_t* text, uint64_t n_bytes);
/* The counts and by_genome_host[n_genomes + 1][SIMMR_BINEVAL_GENOME_COLS] (HOST, either may be NULL).  The bin rows, the cells and
 * the tables are made here, from the records and the assignment that the adds left: a second read gives the same answer, and an
 * add after a read is scored by the next read.  Synchronises (the two scans and the end).  SIMMR_EINVAL: a malformed candidate
 * text since the plan (nothing is written; a malformed truth has no plan).  SIMMR_ESTATE: no truth plan in force. */
int simmr_bineval_read(simmr_bineval* h, simmr_bineval_counts* counts, uint64_t* by_genome_host);
/* The bins of the last read in row order, six columns (DEVICE, capacity entries each, any may be NULL): contigs (u32), bases,
 * none_bases (u64), first_record, top_genome (u32), top_bases (u64).  *n_bins (may be NULL) is written whenever a read holds: a
 * call with capacity 0 asks for it.  Synchronises.  SIMMR_ESTATE: no simmr_bineval_read since the plan or since the last add.
 * SIMMR_ERANGE, no column written: capacity < the bins. */
int simmr_bineval_bins(simmr_bineval* h, uint32_t* contigs_dev, uint64_t* bases_dev, uint64_t* none_bases_dev, uint32_t* first_record_dev,
                       uint32_t* top_genome_dev, uint64_t* top_bases_dev, uint64_t capacity, uint64_t* n_bins);
/* The cells of the last read in (bin, genome) order, four columns (DEVICE, any may be NULL): bin, genome, contigs (u32), bases
 * (u64).  *n_cells, the states and the errors as simmr_bineval_bins. */
int simmr_bineval_cells(simmr_bineval* h, uint32_t* bin_dev, uint32_t* genome_dev, uint32_t* contigs_dev, uint64_t* bases_dev, uint64_t capacity,
                        uint64_t* n_cells);
/* The truth contigs in truth order (add order, then text order), four columns (DEVICE, any may be NULL): the genome row (u32), the
 * length (u64), the bin row of the last read or 0xffffffff (u32), the records that named it (u32).  *n_contigs, the states and the
 * errors as simmr_bineval_bins. */
int simmr_bineval_contigs(simmr_bineval* h, uint32_t* genome_dev, uint64_t* length_dev, uint32_t* bin_dev, uint32_t* records_dev, uint64_t capacity,
                          uint64_t* n_contigs);
/* HIP-event time (ms) of the device work since the last reset: the truth adds, the plans, the adds and the reads.  Synchronises
 * the stream.  A run of adds with no synchronising call of this object between them is timed as one span; the host's wait inside
 * simmr_bineval_add lies inside that span.  *plan_sort_ms (may be NULL) = the sort's share of the last plan. */
int simmr_last_bineval_ms(simmr_bineval* h, float* ms, float* plan_sort_ms);

/* ---- a read error corrector's output scored against the true reads: a SAM text and a FASTQ text in HBM, compared base by base ----
 * Replaces nothing in the reference.  The truth is the text of simmr_sam_emit (either order), or any SAM that follows the rules
 * below: a line carries the read as emitted (SEQ, QUAL), its strand, and in MD:Z the reference base at every mismatch, so the true
 * read is SEQ with MD's letters put in.  The other text is what a corrector (BFC, Lighter, Musket, Karect, ...) made of the run's
 * FASTQ.  No profile changes a read's length and the truth stops at substitutions, so the comparison is position by position and no
 * alignment is made.  No simulation, no genome, no name table: like simmr_mapeval_* without its names.
 *
 * Truth text.  The line rules of simmr_mapeval_truth_add: whole lines of plain SAM, every line ends in '\n' except that the last
 * line of a call may lack it; the caller cuts a file at line ends, at most SIMMR_FIT_SAM_MAX_BYTES a call; an empty line is skipped
 * and not counted; a line that starts with '@' is a header line, counted and skipped.  Every other line is a record, L = the
 * length of SEQ, and goes through these steps in this order:
 *   0. Malformed (sticky): what simmr_mapeval_* calls malformed (fewer than 11 fields; a FLAG, POS or MAPQ that is no number of 1 to
 *      18 digits; a MAPQ above 255; a POS above 2^31 - 1; a CIGAR that is neither "*" nor (<digits><op>)+; an interval that ends
 *      above 2^40).  Nothing of a record can be read before this, so it stands first.
 *   1. Counted truth_skipped: FLAG has 0x100, 0x800 or 0x4; SEQ is "*"; the CIGAR is not exactly one run "<L>M" (1 to 18 digits,
 *      the op 'M' itself).
 *   2. Malformed (sticky): a QNAME that is no read id (1 to 18 decimal digits) or a POS of 0; a QUAL that is neither "*" nor as long
 *      as SEQ, or a QUAL byte outside '!' .. '~'; no "MD:Z:" field among the optional fields (the first one counts); an MD with
 *      '^' or any byte outside the digits and 'A' .. 'Z', or a number of more than 9 digits; MD's matches plus mismatches differ
 *      from L.  (An empty SEQ never gets here: "0M" is no run.)
 *   3. An entry: key = id << 1 | (FLAG & 0x80 ? 1 : 0), L, and per base i of the read IN THE READ'S OWN ORIENTATION (FLAG 0x10:
 *      reversed and complemented, the qualities back to front: the orientation rule of simmr_fit_add_sam) the original class o[i]
 *      (from SEQ), the true class t[i] (MD's letter at a mismatch, o[i] elsewhere) and the quality q[i] = QUAL byte - 33, or 94
 *      where QUAL is "*".  Classes: A C G T in either letter case are 0 .. 3, every other byte is 4; the complement of a class
 *      below 4 is 3 - class, 4 stays.  before = the positions with o != t and t != 4.  RNAME is not resolved.
 *
 * Corrected text.  Records of lines_per_record lines: 4 (FASTQ: '@'name, bases, '+', qualities) or 2 (FASTA: '>'name, bases).
 * Unlike the SAM side EVERY '\n' ends a line, an empty one too, because an empty sequence line is a legal record (a read trimmed
 * to nothing).  The last line of a call may lack its '\n' (a last line that is EMPTY needs it: behind the last '\n' of a call
 * there is no line).  The caller cuts at record ends, at most SIMMR_FIT_SAM_MAX_BYTES a call.  No CRLF (a '\r' is a byte of its
 * line: a base of class 4, a byte of the name) and no records whose bases or qualities run over several lines.  Malformed (sticky):
 * a call whose lines are no multiple of lines_per_record; a first line that does not start with '@' ('>' for two lines); with four
 * lines a third line that does not start with '+', or a fourth line whose length differs from the second's.  The quality line is
 * checked for its length only.
 * Name.  The bytes behind the first character up to the first ' ', '\t' or the line's end, read by the rule of
 * simmr_ovleval_*: 1 to 18 decimal digits, then nothing, "/1" or "/2"; key = id << 1 | ("/2" ? 1 : 0).  A name that is no read
 * name, or a key without an entry, counts unknown_read; every other record is scored (counted `scored`).
 *
 * Verdict.  Lc = the length of the record's bases, c[i] the class of byte i.  For i < min(L, Lc) (the COMPARED positions):
 *   t == 4: ambiguous.   o == t: kept if c == t, else damaged.   o != t: fixed if c == t, left if c == o, else miscorrected.
 * For Lc <= i < L: ambiguous if t == 4, else trimmed_error if o != t, else trimmed_clean.  Only trimming at the 3' end is
 * understood: a read trimmed at its 5' end is compared from its first base like any other, and so is a read whose corrector put
 * in or took out bases in the middle.  Lc > L: extra += Lc - L (longer_records counts the record, trimmed_records one with Lc < L).
 * The nine sums of a record add up to L + extra.  residual = the positions i < L with t != 4 that do not show t (c != t, or
 * i >= Lc), plus extra = damaged + left + miscorrected + trimmed_error + trimmed_clean + extra: 0 means the record is the true read.
 * Tables, over the compared positions: cube[t][o][c] (125 sums, every position); by_qual[q][v] and
 * by_pos[min(i, SIMMR_CORREVAL_POS - 1)][v] with v = 0 kept, 1 damaged, 2 fixed, 3 left, 4 miscorrected (ambiguous positions are
 * in the cube only).
 * Per entry: hits += 1 per scored record, residual = the minimum over its records (0xffffffff: no hit).
 * Every output is an integer sum or minimum: the same for any launch geometry, any cut of either text into adds at line or record
 * ends, and any order of the records. */
#define SIMMR_CORREVAL_POS 512u      /* rows of by_pos: the last one takes every position from 511 on */
#define SIMMR_CORREVAL_QUALS 95u     /* rows of by_qual: 0 .. 93, and 94 for a truth QUAL of "*" */
#define SIMMR_CORREVAL_CLASSES 5u    /* kept, damaged, fixed, left, miscorrected */
#define SIMMR_CORREVAL_NO_HIT 0xffffffffu

typedef struct simmr_correval simmr_correval;

typedef struct simmr_correval_config {   /* HOST memory */
  uint32_t lines_per_record;            /* 4 (FASTQ) or 2 (two-line FASTA); 0: 4 */
  uint32_t reserved;                    /* 0 */
} simmr_correval_config;

typedef struct simmr_correval_counts {   /* HOST; every entry an integer sum, in this order */
  uint64_t truth_lines, truth_header, truth_records, truth_entries, truth_skipped;   /* lines = header + records; cumulative since the reset */
  uint64_t lines, records;                                 /* the corrected side, since the last truth plan */
  uint64_t unknown_read, scored, trimmed_records, longer_records;   /* records = unknown_read + scored */
  uint64_t compared;                                       /* positions: the sum of min(L, Lc), and the sum of the cube */
  uint64_t kept, damaged, fixed, left, miscorrected, ambiguous, trimmed_error, trimmed_clean, extra;   /* bases */
  uint64_t missing, multiple;                              /* truth entries with no hit, with more than one */
  uint64_t clean_kept, clean_damaged;                      /* entries with a hit and before == 0: residual == 0, residual > 0 */
  uint64_t fixed_all, improved, unchanged, worse;          /* before > 0: residual == 0, 0 < residual < before, == before, > before */
} simmr_correval_counts;

/* The state is an object of its own, created on an engine and destroyed BEFORE the engine (as simmr_mapeval_create); its calls
 * run on the engine's stream and leave their messages with the engine (simmr_last_error). */
int simmr_correval_create(simmr_engine* e, simmr_correval** out);
void simmr_correval_destroy(simmr_correval* h);
/* Takes lines_per_record and empties both sides.  Synchronises.  SIMMR_EINVAL: a NULL argument, a lines_per_record other than 0, 2
 * or 4, a reserved word that is not 0. */
int simmr_correval_reset(simmr_correval* h, const simmr_correval_config* cfg);
/* Adds the records of text[0 .. n_bytes) (DEVICE memory, which must stay as it is until the stream has run the add) to the
 * truth.  Only enqueues.  Drops a truth plan.  Room for an entry per 21 bytes of text (no record is shorter) and for a base per
 * byte of text, in two byte planes (o | t << 3, and q), grows with the object.  SIMMR_ESTATE: no reset yet.  SIMMR_EINVAL: a NULL
 * text with n_bytes > 0.  SIMMR_ENOTSUP: n_bytes above SIMMR_FIT_SAM_MAX_BYTES. */
int simmr_correval_truth_add(simmr_correval* h, const uint8_t* text, uint64_t n_bytes);
/* Sorts the entries by key (the radix sort of simmr_sam_sort_plan, over the bits of the largest key), checks that no key stands
 * twice, empties the corrected side and synchronises.  *n_entries (may be NULL) = the entries.  SIMMR_EINVAL: a malformed truth
 * record, or two entries with one key.  SIMMR_ERANGE: 2^31 entries or more. */
int simmr_correval_truth_plan(simmr_correval* h, uint64_t* n_entries);
/* Scores the records of text[0 .. n_bytes) (DEVICE, as above; whole records) against the plan.  Only enqueues.  A line index of
 * four bytes per byte of text grows with the object.  SIMMR_ESTATE: no truth plan in force.  SIMMR_EINVAL, SIMMR_ENOTSUP: as
 * simmr_correval_truth_add. */
int simmr_correval_add(simmr_correval* h, const uint8_t* text, uint64_t n_bytes);
/* The counts, cube_host[5][5][5] ([t][o][c]), by_qual_host[SIMMR_CORREVAL_QUALS][5] and by_pos_host[SIMMR_CORREVAL_POS][5] (HOST,
 * any may be NULL).  Synchronises.  The last eight counts are made here, by a reduction over the entries.  SIMMR_EINVAL: a
 * malformed record on either side since the reset (nothing is written).  SIMMR_ESTATE: no reset yet. */
int simmr_correval_read(simmr_correval* h, simmr_correval_counts* counts, uint64_t* cube_host, uint64_t* by_qual_host, uint64_t* by_pos_host);
/* The truth entries in ascending key order (unique keys: the order is a function of the input), five columns (DEVICE, capacity
 * entries each, any may be NULL): key (u64), length, before, residual (SIMMR_CORREVAL_NO_HIT: no hit), hits (u32).  Synchronises.
 * SIMMR_ESTATE: no truth plan.  SIMMR_ERANGE, nothing written: capacity < n_entries. */
int simmr_correval_emit(simmr_correval* h, uint64_t* key_dev, uint32_t* length_dev, uint32_t* before_dev, uint32_t* residual_dev, uint32_t* hits_dev,
                        uint64_t capacity);
/* HIP-event time (ms) of the device work since the last reset: the adds of either side, the plans and the reads.  Synchronises the
 * stream.  A run of adds with no synchronising call of this object between them is timed as one span. */
int simmr_last_correval_ms(simmr_correval* h, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* SIMMR_HIP_H */
