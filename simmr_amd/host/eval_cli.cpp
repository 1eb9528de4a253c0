// eval_cli.cpp — the eight scorer commands of simmr-hip (--eval-sam, --eval-overlaps, --eval-vcf, --eval-classified, --eval-assembly,
// --eval-placement, --eval-bins, --eval-corrected) over the C ABI of libsimmr_hip.so, and the file walker under them.  None runs a
// simulation; each reads a truth file and a tool's file in pieces, and writes nothing unless all of it succeeded.  What the
// commands share stands first, as plain structs and functions; each command keeps its config, its calls, its tables' sizes, its
// host-side joins and its info lines, and the order of its steps.
#include "eval_cli.hpp"

#include <algorithm>
#include <fstream>
#include <memory>

#include "cli_common.hpp"

using namespace simmr_host;

int file_pieces(const std::string& flag, const std::string& path, PieceCut rule, const std::function<int(const uint8_t*, const char*, size_t)>& add) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return die(flag + ": cannot open " + path);
  struct Closer { FILE* f; ~Closer() { fclose(f); } } closer{f};
  const bool fasta = rule.kind == PieceCut::Fasta;
  PieceReader reader(f, rule, fasta ? SIMMR_ASMEVAL_MAX_BYTES : SIMMR_FIT_SAM_MAX_BYTES);
  GrowBuf dev;
  for (;;) {
    const uint8_t* host = nullptr;
    size_t bytes = 0;
    switch (reader.next(&host, &bytes)) {
      case PieceReader::Piece: break;
      case PieceReader::Done: return 0;
      case PieceReader::CannotRead: return die(flag + ": cannot read " + path);
      case PieceReader::TooLong:
        if (!fasta) return die(flag + ": a " + (rule.kind == PieceCut::Record ? "record" : "line") + " of " + path + " is longer than one add takes");
        fprintf(stderr, "error: %s: a record of %s is longer than one add takes\n", flag.c_str(), path.c_str());
        return 2;
    }
    uint8_t* d = dev.room(bytes);
    if (!d) return die(flag + ": device allocation failed");
    if (hipMemcpy(d, host, bytes, hipMemcpyHostToDevice) != hipSuccess) return die(flag + ": copy to the device failed");
    if (int rc = add(d, (const char*)host, bytes)) return rc;
  }
}

// (a command looks at files before it makes an engine; which of them is the command's own order)
int probe_file(const std::string& flag, const std::string& path) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return die(flag + ": cannot open " + path);
  fclose(f);
  return 0;
}

// The lines in front of a file's records, from which a truth file's names come: the empty ones and those that begin with `mark`.
static bool head_lines(const std::string& path, char mark, std::string* head) {
  std::ifstream in(path, std::ios::binary);
  if (!in) return false;
  for (std::string ln; std::getline(in, ln) && (ln.empty() || ln[0] == mark);) *head += ln + "\n";
  return true;
}

static std::vector<const char*> c_strs(const std::vector<std::string>& v) {
  std::vector<const char*> p;
  for (const std::string& s : v) p.push_back(s.c_str());
  return p;
}

static std::vector<std::string> distinct(std::vector<std::string> v) {
  std::sort(v.begin(), v.end());
  v.erase(std::unique(v.begin(), v.end()), v.end());
  return v;
}

// The engine of a command and the handle of its unit; the handle goes first (the engines are a member, released behind this
// destructor).
template <class H, int (*Create)(simmr_engine*, H**), void (*Destroy)(H*)>
struct Session {
  Engines engines;
  simmr_engine* eng = nullptr;
  H* h = nullptr;
  ~Session() { Destroy(h); }
  int open(const CliArgs& args, const std::string& flag) {
    if (simmr_engine_create(args.device, &eng) != SIMMR_OK) return die(std::string("cannot create engine: ") + simmr_last_error(nullptr));
    engines.v.push_back(eng);
    return Create(eng, &h) != SIMMR_OK ? fail(flag) : 0;
  }
  int fail(const std::string& flag) const { return die(flag + ": " + simmr_last_error(eng)); }
};

// A file through a unit's add, piece by piece; the unit's simmr_last_*_ms behind each add synchronises, so the walker's buffers
// are free for the next piece.
template <class S, class H>
static int add_pieces(const S& s, const std::string& flag, const std::string& path, PieceCut rule, int (*add)(H*, const uint8_t*, uint64_t),
                      int (*last_ms)(H*, float*)) {
  info("Parsing " + path);
  return file_pieces(flag, path, rule, [&](const uint8_t* d, const char*, size_t bytes) {
    float ms = 0;
    return add(s.h, d, bytes) != SIMMR_OK || last_ms(s.h, &ms) != SIMMR_OK ? s.fail(flag) : 0;
  });
}

// The device copies of a truth file's pieces, held until the reset that needs the file's names has been made.
struct KeptPieces {
  struct Piece { GrowBuf dev; size_t bytes = 0; };
  std::vector<std::unique_ptr<Piece>> v;
  int keep(const std::string& flag, const uint8_t* d, size_t bytes) {
    v.emplace_back(new Piece());
    uint8_t* to = v.back()->dev.room(bytes);
    if (!to || hipMemcpy(to, d, bytes, hipMemcpyDeviceToDevice) != hipSuccess) return die(flag + ": device allocation failed");
    v.back()->bytes = bytes;
    return 0;
  }
  template <class S, class H>
  int add_all(const S& s, const std::string& flag, int (*add)(H*, const uint8_t*, uint64_t)) const {
    for (const auto& p : v)
      if (add(s.h, (const uint8_t*)p->dev.p, p->bytes) != SIMMR_OK) return s.fail(flag);
    return 0;
  }
};

// The genome of every record of a gold FASTA: what its first word has in front of the '|'.
static int gold_genomes(const std::string& flag, const std::string& path, const std::vector<std::string>& words, std::vector<std::string>* genomes) {
  for (const std::string& w : words) {
    const size_t bar = w.find('|');
    if (bar == std::string::npos || bar == 0) return die(flag + ": the header '>" + w + "' has no genome in front of a '|': " + path + " is not a file of --gold-assembly");
    genomes->push_back(w.substr(0, bar));
  }
  return 0;
}

// Columns of a unit's rows: `wide` 64-bit and `narrow` 32-bit columns of max(n, 1) rows each (a unit's call takes pointers for no
// rows too), on the device for the call (dw, du) and behind fetch() on the host (w, u).
struct Columns {
  uint64_t rows = 1;
  GrowBuf d_wide, d_narrow;
  std::vector<uint64_t> h_wide;
  std::vector<uint32_t> h_narrow;
  int room(const std::string& flag, size_t wide, size_t narrow, uint64_t n_rows) {
    rows = std::max<uint64_t>(n_rows, 1);
    h_wide.resize(wide * rows);
    h_narrow.resize(narrow * rows);
    if ((wide && !d_wide.room(wide * rows * 8)) || (narrow && !d_narrow.room(narrow * rows * 4))) return die(flag + ": device allocation failed");
    return 0;
  }
  uint64_t* dw(size_t j) const { return (uint64_t*)d_wide.p + j * rows; }
  uint32_t* du(size_t j) const { return (uint32_t*)d_narrow.p + j * rows; }
  int fetch(const std::string& flag) {
    if ((!h_wide.empty() && hipMemcpy(h_wide.data(), d_wide.p, h_wide.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) ||
        (!h_narrow.empty() && hipMemcpy(h_narrow.data(), d_narrow.p, h_narrow.size() * 4, hipMemcpyDeviceToHost) != hipSuccess))
      return die(flag + ": copy from the device failed");
    return 0;
  }
  const uint64_t* w(size_t j) const { return h_wide.data() + j * rows; }
  const uint32_t* u(size_t j) const { return h_narrow.data() + j * rows; }
};

static int write_text(const std::string& flag, const std::string& path, const std::string& text) {
  std::string err;
  OutFile f(path, false);
  f.append(text);
  return f.close(&err) ? 0 : die(flag + ": " + err);
}

static const PieceCut LINES{PieceCut::Newline, 1}, FASTA{PieceCut::Fasta, 1};

// `--eval-sam ALIGNED --eval-truth TRUTH --eval-report OUT`: the names come from the @SQ lines in front of the truth file's records;
// both files go up in pieces, the truth through simmr_mapeval_truth_add and, behind the plan, the aligner's through
// simmr_mapeval_add; the report is written from the counts and by_mapq on the host.
int run_eval_sam(const CliArgs& args) {
  std::vector<std::string> names;
  std::string head;
  if (!head_lines(args.eval_truth, '@', &head)) return die("--eval-truth: cannot open " + args.eval_truth);
  mapeval_sq_names(head.data(), head.size(), &names);
  if (names.empty()) return die("--eval-truth: " + args.eval_truth + " has no @SQ lines in front of its records: the sequences' names come from them");
  if (int rc = probe_file("--eval-sam", args.eval_sam)) return rc;
  Session<simmr_mapeval, simmr_mapeval_create, simmr_mapeval_destroy> ev;
  if (int rc = ev.open(args, "--eval-sam")) return rc;
  std::vector<const char*> rname = c_strs(names);
  const simmr_mapeval_config cfg{(uint32_t)rname.size(), args.eval_min_overlap, rname.data()};
  if (simmr_mapeval_reset(ev.h, &cfg) != SIMMR_OK) return ev.fail("--eval-truth");
  if (int rc = add_pieces(ev, "--eval-truth", args.eval_truth, LINES, simmr_mapeval_truth_add, simmr_last_mapeval_ms)) return rc;
  uint64_t n_entries = 0;
  if (simmr_mapeval_truth_plan(ev.h, &n_entries) != SIMMR_OK) return ev.fail("--eval-truth");
  if (int rc = add_pieces(ev, "--eval-sam", args.eval_sam, LINES, simmr_mapeval_add, simmr_last_mapeval_ms)) return rc;
  simmr_mapeval_counts c{};
  static_assert(sizeof(c) == MAPEVAL_N_COUNTS * sizeof(uint64_t), "the report names every count");
  std::vector<uint64_t> by_mapq(512);
  if (simmr_mapeval_read(ev.h, &c, by_mapq.data()) != SIMMR_OK) return ev.fail("--eval-sam");
  std::string rows;
  if (!args.eval_reads.empty()) {
    Columns cols;  // key; best, hits
    if (int rc = cols.room("--eval-reads", 1, 2, n_entries)) return rc;
    if (simmr_mapeval_emit(ev.h, cols.dw(0), cols.du(0), cols.du(1), n_entries) != SIMMR_OK) return ev.fail("--eval-reads");
    if (int rc = cols.fetch("--eval-reads")) return rc;
    rows = mapeval_read_rows(cols.w(0), cols.u(0), cols.u(1), n_entries);
  }
  if (int rc = write_text("--eval-report", args.eval_report, mapeval_report((const uint64_t*)&c, by_mapq.data()))) return rc;
  if (!args.eval_reads.empty())
    if (int rc = write_text("--eval-reads", args.eval_reads, rows)) return rc;
  info("Truth: " + n(c.truth_entries) + " reads (" + n(c.truth_skipped) + " records skipped)");
  info("Aligned: " + n(c.records) + " records: " + n(c.correct) + " correct, " + n(c.wrong) + " wrong, " + n(c.unmapped) + " unmapped; " + n(c.secondary) +
       " secondary or supplementary, " + n(c.cigar_op) + " with an operation other than M = X I D S H, " + n(c.unknown_read) + " of unknown reads");
  info("Reads: " + n(c.reads_correct) + " correct, " + n(c.reads_wrong) + " wrong, " + n(c.reads_unmapped) + " unmapped, " + n(c.missing) + " without a record");
  info("Wrote " + args.eval_report);
  return 0;
}

// `--eval-overlaps CANDIDATE --eval-overlaps-truth TRUTH --eval-overlaps-report OUT`: both files go up in pieces, the truth through
// simmr_ovleval_truth_add and, behind the plan, the overlapper's through simmr_ovleval_add; the report is written from the counts
// and by_len on the host.
int run_eval_overlaps(const CliArgs& args) {
  if (int rc = probe_file("--eval-overlaps-truth", args.eval_overlaps_truth)) return rc;
  if (int rc = probe_file("--eval-overlaps", args.eval_overlaps)) return rc;
  Session<simmr_ovleval, simmr_ovleval_create, simmr_ovleval_destroy> ev;
  if (int rc = ev.open(args, "--eval-overlaps")) return rc;
  if (simmr_ovleval_reset(ev.h, args.eval_overlaps_min_pct) != SIMMR_OK) return ev.fail("--eval-overlaps");
  if (int rc = add_pieces(ev, "--eval-overlaps-truth", args.eval_overlaps_truth, LINES, simmr_ovleval_truth_add, simmr_last_ovleval_ms)) return rc;
  uint64_t n_entries = 0, n_reads = 0;
  if (simmr_ovleval_truth_plan(ev.h, &n_entries, &n_reads) != SIMMR_OK) return ev.fail("--eval-overlaps-truth");
  if (int rc = add_pieces(ev, "--eval-overlaps", args.eval_overlaps, LINES, simmr_ovleval_add, simmr_last_ovleval_ms)) return rc;
  simmr_ovleval_counts c{};
  static_assert(sizeof(c) == OVLEVAL_N_COUNTS * sizeof(uint64_t) && OVLEVAL_LEN_ROWS == SIMMR_OVLEVAL_LEN_ROWS, "the report names every count and row");
  std::vector<uint64_t> by_len(2 * OVLEVAL_LEN_ROWS);
  if (simmr_ovleval_read(ev.h, &c, by_len.data()) != SIMMR_OK) return ev.fail("--eval-overlaps");
  std::string rows;
  if (!args.eval_overlaps_pairs.empty()) {
    Columns cols;  // key_a, key_b, ov; best, hits
    if (int rc = cols.room("--eval-overlaps-pairs", 3, 2, n_entries)) return rc;
    if (simmr_ovleval_emit(ev.h, cols.dw(0), cols.dw(1), cols.dw(2), cols.du(0), cols.du(1), n_entries) != SIMMR_OK) return ev.fail("--eval-overlaps-pairs");
    if (int rc = cols.fetch("--eval-overlaps-pairs")) return rc;
    rows = ovleval_pair_rows(cols.w(0), cols.w(1), cols.w(2), cols.u(0), cols.u(1), n_entries);
  }
  if (int rc = write_text("--eval-overlaps-report", args.eval_overlaps_report, ovleval_report((const uint64_t*)&c, by_len.data()))) return rc;
  if (!args.eval_overlaps_pairs.empty())
    if (int rc = write_text("--eval-overlaps-pairs", args.eval_overlaps_pairs, rows)) return rc;
  info("Truth: " + n(c.truth_entries) + " pairs of " + n(c.truth_reads) + " reads");
  info("Candidate: " + n(c.records) + " records: " + n(c.correct) + " correct, " + n(c.wrong) + " wrong (" + n(c.unknown_read) + " of unknown reads, " +
       n(c.no_pair) + " of pairs that do not overlap, " + n(c.wrong_strand) + " on the other strand, " + n(c.wrong_interval) + " off the interval), " +
       n(c.self) + " of a read with itself");
  info("Pairs: " + n(c.pairs_found) + " found, " + n(c.pairs_wrong) + " reported wrong only, " + n(c.pairs_missed) + " missed, " + n(c.pairs_multiple) +
       " reported more than once");
  info("Wrote " + args.eval_overlaps_report);
  return 0;
}

// `--eval-vcf CALLS --eval-vcf-truth TRUTH --eval-vcf-report OUT`: the names come from the ##contig lines in front of the truth
// file's records; both files go up in pieces, the truth through simmr_vcfeval_truth_add and, behind the plan, the caller's through
// simmr_vcfeval_add; the report is written from the counts, by_qual and by_ad on the host.
int run_eval_vcf(const CliArgs& args) {
  std::vector<std::string> names;
  std::string head;
  if (!head_lines(args.eval_vcf_truth, '#', &head)) return die("--eval-vcf-truth: cannot open " + args.eval_vcf_truth);
  vcfeval_contig_names(head.data(), head.size(), &names);
  if (names.empty()) return die("--eval-vcf-truth: " + args.eval_vcf_truth + " has no ##contig=<ID=...> lines in front of its records: the contigs' names come from them");
  if (int rc = probe_file("--eval-vcf", args.eval_vcf)) return rc;
  Session<simmr_vcfeval, simmr_vcfeval_create, simmr_vcfeval_destroy> ev;
  if (int rc = ev.open(args, "--eval-vcf")) return rc;
  std::vector<const char*> rname = c_strs(names);
  const simmr_vcfeval_config cfg{(uint32_t)rname.size(), args.eval_vcf_filtered ? 1u : 0u, rname.data()};
  if (simmr_vcfeval_reset(ev.h, &cfg) != SIMMR_OK) return ev.fail("--eval-vcf-truth");
  if (int rc = add_pieces(ev, "--eval-vcf-truth", args.eval_vcf_truth, LINES, simmr_vcfeval_truth_add, simmr_last_vcfeval_ms)) return rc;
  uint64_t n_entries = 0;
  if (simmr_vcfeval_truth_plan(ev.h, &n_entries) != SIMMR_OK) return ev.fail("--eval-vcf-truth");
  if (int rc = add_pieces(ev, "--eval-vcf", args.eval_vcf, LINES, simmr_vcfeval_add, simmr_last_vcfeval_ms)) return rc;
  simmr_vcfeval_counts c{};
  static_assert(sizeof(c) == VCFEVAL_N_COUNTS * sizeof(uint64_t) && VCFEVAL_AD_ROWS == SIMMR_VCFEVAL_AD_ROWS, "the report names every count and row");
  std::vector<uint64_t> by_qual(512), by_ad(2 * VCFEVAL_AD_ROWS);
  if (simmr_vcfeval_read(ev.h, &c, by_qual.data(), by_ad.data()) != SIMMR_OK) return ev.fail("--eval-vcf");
  std::string rows;
  if (!args.eval_vcf_sites.empty()) {
    Columns cols;  // key; alleles, ad, best, hits
    if (int rc = cols.room("--eval-vcf-sites", 1, 4, n_entries)) return rc;
    if (simmr_vcfeval_emit(ev.h, cols.dw(0), cols.du(0), cols.du(1), cols.du(2), cols.du(3), n_entries) != SIMMR_OK) return ev.fail("--eval-vcf-sites");
    if (int rc = cols.fetch("--eval-vcf-sites")) return rc;
    std::sort(names.begin(), names.end());  // (the rows of the key are places in the sorted names)
    rows = vcfeval_site_rows(names, cols.w(0), cols.u(0), cols.u(1), cols.u(2), cols.u(3), n_entries);
  }
  if (int rc = write_text("--eval-vcf-report", args.eval_vcf_report, vcfeval_report((const uint64_t*)&c, by_qual.data(), by_ad.data()))) return rc;
  if (!args.eval_vcf_sites.empty())
    if (int rc = write_text("--eval-vcf-sites", args.eval_vcf_sites, rows)) return rc;
  info("Truth: " + n(c.truth_entries) + " sites");
  info("Calls: " + n(c.records) + " records (" + n(c.filtered) + " filtered, " + n(c.ref_call) + " reference calls): " + n(c.calls) + " calls, " + n(c.correct) +
       " correct, " + n(c.wrong) + " wrong (" + n(c.unknown_contig) + " on unknown contigs, " + n(c.no_site) + " where no site is, " + n(c.ref_mismatch) +
       " with another reference base, " + n(c.wrong_allele) + " with another allele); " + n(c.indel) + " indel, " + n(c.symbolic) + " symbolic and " +
       n(c.long_allele) + " long alleles not scored");
  info("Sites: " + n(c.sites_found) + " found, " + n(c.sites_wrong) + " called wrong only, " + n(c.sites_missed) + " missed, " + n(c.sites_multiple) +
       " called more than once");
  info("Wrote " + args.eval_vcf_report);
  return 0;
}

// `--eval-classified CALLS --eval-classified-truth TRUTH --eval-taxonomy NODES --eval-genome-taxa MAP --eval-classified-report OUT`:
// the two small files are parsed here and handed to simmr_taxeval_reset; both big files go up in pieces, the truth through
// simmr_taxeval_truth_add and, behind the plan, the classifier's through simmr_taxeval_add; the three texts are written from the
// integer tables on the host.
static bool slurp(const std::string& path, std::string* out) {
  std::ifstream in(path, std::ios::binary);
  if (!in) return false;
  out->assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
  return true;
}
int run_eval_classified(const CliArgs& args) {
  std::string text, perr;
  std::vector<uint32_t> taxid, parent, gtax;
  std::vector<uint8_t> rank;
  std::vector<std::string> gid;
  if (!slurp(args.eval_taxonomy, &text)) return die("--eval-taxonomy: cannot open " + args.eval_taxonomy);
  if (!taxeval_parse_nodes(text.data(), text.size(), &taxid, &parent, &rank, &perr)) return die("--eval-taxonomy: " + args.eval_taxonomy + ": " + perr);
  if (!slurp(args.eval_genome_taxa, &text)) return die("--eval-genome-taxa: cannot open " + args.eval_genome_taxa);
  if (!taxeval_parse_map(text.data(), text.size(), &gid, &gtax, &perr)) return die("--eval-genome-taxa: " + args.eval_genome_taxa + ": " + perr);
  text.clear();
  if (int rc = probe_file("--eval-classified-truth", args.eval_classified_truth)) return rc;
  if (int rc = probe_file("--eval-classified", args.eval_classified)) return rc;
  Session<simmr_taxeval, simmr_taxeval_create, simmr_taxeval_destroy> ev;
  if (int rc = ev.open(args, "--eval-classified")) return rc;
  std::vector<const char*> ids = c_strs(gid);
  const simmr_taxeval_config cfg{taxid.size(), taxid.data(), parent.data(), rank.data(), gid.size(), ids.data(), gtax.data()};
  if (simmr_taxeval_reset(ev.h, &cfg) != SIMMR_OK) return ev.fail("--eval-taxonomy");
  if (int rc = add_pieces(ev, "--eval-classified-truth", args.eval_classified_truth, LINES, simmr_taxeval_truth_add, simmr_last_taxeval_ms)) return rc;
  uint64_t n_entries = 0;
  if (simmr_taxeval_truth_plan(ev.h, &n_entries) != SIMMR_OK) return ev.fail("--eval-classified-truth");
  if (int rc = add_pieces(ev, "--eval-classified", args.eval_classified, LINES, simmr_taxeval_add, simmr_last_taxeval_ms)) return rc;
  simmr_taxeval_counts c{};
  static_assert(sizeof(c) == TAXEVAL_N_COUNTS * sizeof(uint64_t) && TAXEVAL_RANKS == SIMMR_TAXEVAL_RANKS && TAXEVAL_CLASSES == SIMMR_TAXEVAL_CLASSES,
                "the report names every count, rank and class");
  std::vector<uint64_t> by_rank(TAXEVAL_RANKS * TAXEVAL_CLASSES), reads_by_rank(TAXEVAL_RANKS * TAXEVAL_CLASSES);
  if (simmr_taxeval_read(ev.h, &c, by_rank.data(), reads_by_rank.data()) != SIMMR_OK) return ev.fail("--eval-classified");
  // the per-taxon rows: the clade sums in taxid order, and the ranks put into that order here
  const uint64_t nn = taxid.size();
  Columns taxa;  // true, called, both; taxid
  if (int rc = taxa.room("--eval-classified", 3, 1, nn)) return rc;
  if (simmr_taxeval_taxa(ev.h, taxa.du(0), taxa.dw(0), taxa.dw(1), taxa.dw(2), nn) != SIMMR_OK) return ev.fail("--eval-classified");
  if (int rc = taxa.fetch("--eval-classified")) return rc;
  std::vector<uint32_t> order(nn);
  for (uint32_t i = 0; i < nn; i++) order[i] = i;
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return taxid[a] < taxid[b]; });
  std::vector<uint8_t> s_rank(taxa.rows, 0);
  for (uint64_t i = 0; i < nn; i++) s_rank[i] = rank[order[i]];
  std::string rows;
  if (!args.eval_classified_reads.empty()) {
    // a genome's row is its place among the sorted ids; the ranks its lineage has come from simmr_taxeval_lineage
    std::vector<uint32_t> g_order(gid.size());
    for (uint32_t i = 0; i < gid.size(); i++) g_order[i] = i;
    std::sort(g_order.begin(), g_order.end(), [&](uint32_t a, uint32_t b) { return gid[a] < gid[b]; });
    std::vector<std::string> s_gid;
    std::vector<uint32_t> has;
    for (uint32_t g : g_order) {
      uint32_t lin[TAXEVAL_RANKS] = {}, mask = 0;
      if (simmr_taxeval_lineage(ev.h, gtax[g], lin, nullptr) != SIMMR_OK) return ev.fail("--eval-classified-reads");
      for (size_t r = 0; r < TAXEVAL_RANKS; r++) mask |= lin[r] ? 1u << r : 0u;
      s_gid.push_back(gid[g]);
      has.push_back(mask);
    }
    Columns cols;  // id; genome, mates, seen, hits
    if (int rc = cols.room("--eval-classified-reads", 1, 4, n_entries)) return rc;
    if (simmr_taxeval_emit(ev.h, cols.dw(0), cols.du(0), cols.du(1), cols.du(2), cols.du(3), n_entries) != SIMMR_OK) return ev.fail("--eval-classified-reads");
    if (int rc = cols.fetch("--eval-classified-reads")) return rc;
    rows = taxeval_read_rows(s_gid, has, cols.w(0), cols.u(0), cols.u(1), cols.u(2), cols.u(3), n_entries);
  }
  if (int rc = write_text("--eval-classified-report", args.eval_classified_report,
                          taxeval_report((const uint64_t*)&c, by_rank.data(), reads_by_rank.data(), s_rank.data(), taxa.w(0), taxa.w(1), nn)))
    return rc;
  if (!args.eval_classified_reads.empty())
    if (int rc = write_text("--eval-classified-reads", args.eval_classified_reads, rows)) return rc;
  if (!args.eval_classified_taxa.empty())
    if (int rc = write_text("--eval-classified-taxa", args.eval_classified_taxa, taxeval_taxa_rows(taxa.u(0), s_rank.data(), taxa.w(0), taxa.w(1), taxa.w(2), nn)))
      return rc;
  info("Truth: " + n(c.truth_entries) + " reads (" + n(c.truth_paired) + " paired) of " + n(gid.size()) + " genomes; " + n(nn) + " taxa");
  info("Calls: " + n(c.records) + " records: " + n(c.scored) + " scored, " + n(c.unclassified) + " unclassified, " + n(c.unknown_taxon) +
       " with a taxid that is no node, " + n(c.unknown_read) + " of unknown reads");
  info("Reads: " + n(c.missing) + " without a record, " + n(c.multiple) + " with more records than lines");
  info("Wrote " + args.eval_classified_report);
  return 0;
}

// `--eval-assembly CONTIGS.fa --eval-assembly-truth GOLD.fa --eval-assembly-report OUT`: a FASTA file goes to the device in pieces of
// whole records (PieceCut::Fasta).  The host reads every piece once for the records' first words and lengths: the genomes are the
// distinct prefixes of the truth's first words, so the truth's pieces are kept on the device until the reset, which needs them.
int run_eval_assembly(const CliArgs& args) {
  if (int rc = probe_file("--eval-assembly", args.eval_assembly)) return rc;
  Session<simmr_asmeval, simmr_asmeval_create, simmr_asmeval_destroy> ev;
  if (int rc = ev.open(args, "--eval-assembly")) return rc;
  std::vector<std::string> t_words, c_words, t_genome;
  std::vector<uint64_t> t_len, c_len_host;
  KeptPieces kept;
  info("Parsing " + args.eval_assembly_truth);
  if (int rc = file_pieces("--eval-assembly-truth", args.eval_assembly_truth, FASTA, [&](const uint8_t* d, const char* host, size_t bytes) {
        asmeval_fasta_records(host, bytes, &t_words, &t_len);
        return kept.keep("--eval-assembly-truth", d, bytes);
      }))
    return rc;
  if (int rc = gold_genomes("--eval-assembly-truth", args.eval_assembly_truth, t_words, &t_genome)) return rc;
  const std::vector<std::string> genomes = distinct(t_genome);
  std::vector<const char*> gname = c_strs(genomes);
  const simmr_asmeval_config cfg{(uint32_t)gname.size(), args.eval_assembly_k, 0u, gname.data()};
  if (simmr_asmeval_reset(ev.h, &cfg) != SIMMR_OK) return ev.fail("--eval-assembly-truth");
  if (int rc = kept.add_all(ev, "--eval-assembly-truth", simmr_asmeval_truth_add)) return rc;
  uint64_t n_entries = 0;
  if (simmr_asmeval_truth_plan(ev.h, &n_entries) != SIMMR_OK) return ev.fail("--eval-assembly-truth");
  kept.v.clear();
  info("Parsing " + args.eval_assembly);
  if (int rc = file_pieces("--eval-assembly", args.eval_assembly, FASTA, [&](const uint8_t* d, const char* host, size_t bytes) {
        asmeval_fasta_records(host, bytes, &c_words, &c_len_host);
        return simmr_asmeval_add(ev.h, d, bytes) != SIMMR_OK ? ev.fail("--eval-assembly") : 0;  // (synchronises)
      }))
    return rc;
  simmr_asmeval_counts c{};
  static_assert(sizeof(c) == ASMEVAL_N_COUNTS * sizeof(uint64_t) && ASMEVAL_GENOME_COLS == SIMMR_ASMEVAL_GENOME_COLS, "the report names every count and column");
  std::vector<uint64_t> by_genome((genomes.size() + 1) * ASMEVAL_GENOME_COLS);
  if (simmr_asmeval_read(ev.h, &c, by_genome.data()) != SIMMR_OK) return ev.fail("--eval-assembly");
  const uint64_t nc = c.records;
  Columns cols;  // length; kmers, found, shared, top_genome, top_kmers
  if (int rc = cols.room("--eval-assembly", 1, 5, nc)) return rc;
  if (simmr_asmeval_contigs(ev.h, cols.dw(0), cols.du(0), cols.du(1), cols.du(2), cols.du(3), cols.du(4), nc, nullptr) != SIMMR_OK) return ev.fail("--eval-assembly");
  if (int rc = cols.fetch("--eval-assembly")) return rc;
  if (int rc = write_text("--eval-assembly-report", args.eval_assembly_report,
                          asmeval_report((const uint64_t*)&c, args.eval_assembly_k, genomes, by_genome.data(), t_len.data(), t_len.size(), cols.w(0), nc)))
    return rc;
  if (!args.eval_assembly_contigs.empty())
    if (int rc = write_text("--eval-assembly-contigs", args.eval_assembly_contigs,
                            asmeval_contig_rows(c_words, genomes, cols.w(0), cols.u(0), cols.u(1), cols.u(2), cols.u(3), cols.u(4), nc)))
      return rc;
  info("Truth: " + n(c.truth_records) + " records, " + n(c.truth_bases) + " bases, " + n(n_entries) + " distinct " + std::to_string(args.eval_assembly_k) + "-mers of " +
       n(genomes.size()) + " genomes (" + n(c.truth_shared_distinct) + " in more than one)");
  info("Contigs: " + n(c.records) + " records, " + n(c.bases) + " bases, " + n(c.kmers) + " k-mers: " + n(c.found) + " found, " + n(c.novel) + " in no genome; " +
       n(c.contigs_pure) + " pure, " + n(c.contigs_mixed) + " mixed, " + n(c.contigs_novel) + " novel, " + n(c.contigs_shared_only) + " shared only, " +
       n(c.contigs_short) + " shorter than k");
  info("Wrote " + args.eval_assembly_report);
  return 0;
}

// `--eval-placement CONTIGS.fa --eval-placement-truth GOLD.fa --eval-placement-report OUT`: the files and the genome names are read
// exactly as --eval-assembly reads them; the host keeps the first words of both sides for the block rows and computes NA50 / NGA50
// from the block columns, as it computes N50 there.
int run_eval_placement(const CliArgs& args) {
  if (int rc = probe_file("--eval-placement", args.eval_placement)) return rc;
  Session<simmr_asmmap, simmr_asmmap_create, simmr_asmmap_destroy> ev;
  if (int rc = ev.open(args, "--eval-placement")) return rc;
  std::vector<std::string> t_words, c_words, t_genome_name;  // (the last: per truth record)
  std::vector<uint64_t> t_len, c_len_host;
  KeptPieces kept;
  info("Parsing " + args.eval_placement_truth);
  if (int rc = file_pieces("--eval-placement-truth", args.eval_placement_truth, FASTA, [&](const uint8_t* d, const char* host, size_t bytes) {
        asmeval_fasta_records(host, bytes, &t_words, &t_len);
        return kept.keep("--eval-placement-truth", d, bytes);
      }))
    return rc;
  if (int rc = gold_genomes("--eval-placement-truth", args.eval_placement_truth, t_words, &t_genome_name)) return rc;
  const std::vector<std::string> genomes = distinct(t_genome_name);
  std::vector<const char*> gname = c_strs(genomes);
  const simmr_asmmap_config cfg{(uint32_t)gname.size(), args.eval_placement_k, args.eval_placement_band, args.eval_placement_relocation,
                                args.eval_placement_min_anchors, gname.data()};
  if (simmr_asmmap_reset(ev.h, &cfg) != SIMMR_OK) return ev.fail("--eval-placement-truth");
  if (int rc = kept.add_all(ev, "--eval-placement-truth", simmr_asmmap_truth_add)) return rc;
  uint64_t n_anchors = 0;
  if (simmr_asmmap_truth_plan(ev.h, &n_anchors) != SIMMR_OK) return ev.fail("--eval-placement-truth");
  kept.v.clear();
  info("Parsing " + args.eval_placement);
  if (int rc = file_pieces("--eval-placement", args.eval_placement, FASTA, [&](const uint8_t* d, const char* host, size_t bytes) {
        asmeval_fasta_records(host, bytes, &c_words, &c_len_host);
        return simmr_asmmap_add(ev.h, d, bytes) != SIMMR_OK ? ev.fail("--eval-placement") : 0;  // (synchronises)
      }))
    return rc;
  simmr_asmmap_counts c{};
  static_assert(sizeof(c) == ASMMAP_N_COUNTS * sizeof(uint64_t) && ASMMAP_GENOME_COLS == SIMMR_ASMMAP_GENOME_COLS && ASMMAP_BLOCK_COLS == SIMMR_ASMMAP_BLOCK_COLS,
                "the report names every count and column");
  std::vector<uint64_t> by_genome(std::max<size_t>(genomes.size(), 1) * ASMMAP_GENOME_COLS);
  if (simmr_asmmap_read(ev.h, &c, by_genome.data()) != SIMMR_OK) return ev.fail("--eval-placement");
  const uint64_t nb = c.blocks, nc = c.records;
  Columns blocks, contigs;  // the nine block columns; length, block_bases; hits, blocks, first_block, worst_join
  if (blocks.room("--eval-placement", 0, ASMMAP_BLOCK_COLS, nb) || contigs.room("--eval-placement", 2, 4, nc)) return 1;
  uint32_t* bcols[ASMMAP_BLOCK_COLS];
  const uint32_t* hcols[ASMMAP_BLOCK_COLS];
  for (size_t j = 0; j < ASMMAP_BLOCK_COLS; j++) bcols[j] = blocks.du(j), hcols[j] = blocks.u(j);
  if (simmr_asmmap_blocks(ev.h, bcols, nb, nullptr) != SIMMR_OK) return ev.fail("--eval-placement");
  if (simmr_asmmap_contigs(ev.h, contigs.dw(0), contigs.du(0), contigs.du(1), contigs.du(2), contigs.dw(1), contigs.du(3), nc, nullptr) != SIMMR_OK)
    return ev.fail("--eval-placement");
  if (blocks.fetch("--eval-placement") || contigs.fetch("--eval-placement")) return 1;
  std::vector<uint64_t> block_length(nb);
  std::vector<uint32_t> block_genome(nb);
  for (uint64_t i = 0; i < nb; i++) {
    block_length[i] = hcols[4][i] - hcols[3][i];
    const uint32_t t = hcols[1][i];
    block_genome[i] = t < t_genome_name.size() ? (uint32_t)(std::lower_bound(genomes.begin(), genomes.end(), t_genome_name[t]) - genomes.begin()) : 0xffffffffu;
  }
  if (int rc = write_text("--eval-placement-report", args.eval_placement_report,
                          asmmap_report((const uint64_t*)&c, args.eval_placement_k, args.eval_placement_band, args.eval_placement_relocation,
                                        args.eval_placement_min_anchors, genomes, by_genome.data(), block_length.data(), block_genome.data(), nb)))
    return rc;
  if (!args.eval_placement_blocks.empty())
    if (int rc = write_text("--eval-placement-blocks", args.eval_placement_blocks, asmmap_block_rows(c_words, t_words, hcols, nb))) return rc;
  if (!args.eval_placement_contigs.empty())
    if (int rc = write_text("--eval-placement-contigs", args.eval_placement_contigs,
                            asmmap_contig_rows(c_words, contigs.w(0), contigs.u(0), contigs.u(1), contigs.u(2), contigs.w(1), contigs.u(3), nc)))
      return rc;
  info("Truth: " + n(c.truth_records) + " records, " + n(c.truth_bases) + " bases, " + n(n_anchors) + " unique " + std::to_string(args.eval_placement_k) + "-mers of " +
       n(genomes.size()) + " genomes as anchors (" + n(c.truth_repeats) + " repeated)");
  info("Contigs: " + n(c.records) + " records, " + n(c.bases) + " bases, " + n(c.hits) + " anchor hits in " + n(c.blocks) + " blocks; " +
       n(c.breaks_inter_genome + c.breaks_inter_record + c.breaks_inversion + c.breaks_relocation) + " misassemblies in " + n(c.contigs_misassembled) + " contigs, " +
       n(c.breaks_local) + " local breaks, " + n(c.contigs_unplaced) + " contigs unplaced");
  info("Wrote " + args.eval_placement_report);
  return 0;
}

// `--eval-bins BINS.tsv --eval-bins-truth CONTIGS.tsv --eval-bins-report OUT`: both files go up in pieces cut at the last newline.
// The host reads every piece once for the names: the truth's contig names and its genomes (the distinct field-8 values other than
// "."), so the truth's pieces are kept on the device until the reset, which needs them; the records' bin names, of which a bin's
// name is the one at its first_record.
int run_eval_bins(const CliArgs& args) {
  if (int rc = probe_file("--eval-bins", args.eval_bins)) return rc;
  Session<simmr_bineval, simmr_bineval_create, simmr_bineval_destroy> ev;
  if (int rc = ev.open(args, "--eval-bins")) return rc;
  std::vector<std::string> t_names, t_genomes, r_bins;
  KeptPieces kept;
  info("Parsing " + args.eval_bins_truth);
  if (int rc = file_pieces("--eval-bins-truth", args.eval_bins_truth, LINES, [&](const uint8_t* d, const char* host, size_t bytes) {
        if (int rc = kept.keep("--eval-bins-truth", d, bytes)) return rc;
        bineval_truth_names(host, bytes, &t_names, &t_genomes);
        return 0;
      }))
    return rc;
  std::vector<std::string> genomes;
  for (const std::string& g : t_genomes)
    if (g != "." && !g.empty()) genomes.push_back(g);
  std::vector<std::string>().swap(t_genomes);
  genomes = distinct(std::move(genomes));
  std::vector<const char*> gname = c_strs(genomes);
  const simmr_bineval_config cfg{(uint32_t)gname.size(), 64u, gname.data()};
  if (simmr_bineval_reset(ev.h, &cfg) != SIMMR_OK) return ev.fail("--eval-bins-truth");
  if (int rc = kept.add_all(ev, "--eval-bins-truth", simmr_bineval_truth_add)) return rc;
  uint64_t n_truth = 0;
  if (simmr_bineval_truth_plan(ev.h, &n_truth) != SIMMR_OK) return ev.fail("--eval-bins-truth");
  kept.v.clear();
  info("Parsing " + args.eval_bins);
  if (int rc = file_pieces("--eval-bins", args.eval_bins, LINES, [&](const uint8_t* d, const char* host, size_t bytes) {
        if (simmr_bineval_add(ev.h, d, bytes) != SIMMR_OK) return ev.fail("--eval-bins");
        // (the device is waited for: it ends behind the add's lookups, so the walker may reuse the buffer)
        if (hipDeviceSynchronize() != hipSuccess) return die("--eval-bins: copy from the device failed");
        bineval_record_bins(host, bytes, &r_bins);
        return 0;
      }))
    return rc;
  simmr_bineval_counts c{};
  static_assert(sizeof(c) == BINEVAL_N_COUNTS * sizeof(uint64_t) && BINEVAL_GENOME_COLS == SIMMR_BINEVAL_GENOME_COLS, "the report names every count and column");
  std::vector<uint64_t> by_genome((genomes.size() + 1) * BINEVAL_GENOME_COLS);
  if (simmr_bineval_read(ev.h, &c, by_genome.data()) != SIMMR_OK) return ev.fail("--eval-bins");
  const uint64_t nb = c.bins, nc = c.cells, nt = c.truth_records;
  // bases, none_bases, top_bases; contigs, first_record, top_genome / bases; bin, genome, contigs / length; genome, bin, records
  Columns bins, cells, contigs;
  if (bins.room("--eval-bins", 3, 3, nb) || cells.room("--eval-bins", 1, 3, nc) || contigs.room("--eval-bins", 1, 3, nt)) return 1;
  if (simmr_bineval_bins(ev.h, bins.du(0), bins.dw(0), bins.dw(1), bins.du(1), bins.du(2), bins.dw(2), nb, nullptr) != SIMMR_OK ||
      simmr_bineval_cells(ev.h, cells.du(0), cells.du(1), cells.du(2), cells.dw(0), nc, nullptr) != SIMMR_OK ||
      simmr_bineval_contigs(ev.h, contigs.du(0), contigs.dw(0), contigs.du(1), contigs.du(2), nt, nullptr) != SIMMR_OK)
    return ev.fail("--eval-bins");
  if (bins.fetch("--eval-bins") || cells.fetch("--eval-bins") || contigs.fetch("--eval-bins")) return 1;
  std::vector<std::string> bin_names;
  for (uint64_t b = 0; b < nb; b++) {
    const uint32_t first = bins.u(1)[b];
    bin_names.push_back(first < r_bins.size() ? r_bins[first] : std::string("?"));
  }
  if (int rc = write_text("--eval-bins-report", args.eval_bins_report,
                          bineval_report((const uint64_t*)&c, genomes, by_genome.data(), bin_names, bins.u(0), bins.w(0), bins.w(1), bins.u(2), bins.w(2), nb)))
    return rc;
  if (!args.eval_bins_bins.empty())
    if (int rc = write_text("--eval-bins-bins", args.eval_bins_bins, bineval_cell_rows(bin_names, genomes, cells.u(0), cells.u(1), cells.u(2), cells.w(0), nc))) return rc;
  if (!args.eval_bins_contigs.empty())
    if (int rc = write_text("--eval-bins-contigs", args.eval_bins_contigs,
                            bineval_contig_rows(t_names, genomes, bin_names, contigs.u(0), contigs.w(0), contigs.u(1), contigs.u(2), nt)))
      return rc;
  info("Truth: " + n(c.truth_records) + " contigs, " + n(c.truth_bases) + " bases of " + n(genomes.size()) + " genomes (" + n(c.truth_none) + " contigs of none)");
  info("Bins: " + n(c.records) + " records: " + n(c.unknown_contig) + " of unknown contigs, " + n(c.repeated) + " repeated; " + n(c.assigned) + " contigs in " +
       n(c.bins) + " bins, " + n(c.cells) + " cells");
  info("Wrote " + args.eval_bins_report);
  return 0;
}

// `--eval-corrected READS.fastq --eval-corrected-truth TRUTH.sam --eval-corrected-report OUT`: the truth goes up in pieces cut at the
// last newline through simmr_correval_truth_add; behind the plan the reads go up in pieces cut at a record's end (PieceCut::Record
// of four lines, or two with --eval-corrected-fasta) through simmr_correval_add.
int run_eval_corrected(const CliArgs& args) {
  if (int rc = probe_file("--eval-corrected-truth", args.eval_corrected_truth)) return rc;
  if (int rc = probe_file("--eval-corrected", args.eval_corrected)) return rc;
  Session<simmr_correval, simmr_correval_create, simmr_correval_destroy> ev;
  if (int rc = ev.open(args, "--eval-corrected")) return rc;
  const uint32_t lpr = args.eval_corrected_fasta ? 2u : 4u;
  const simmr_correval_config cfg{lpr, 0u};
  if (simmr_correval_reset(ev.h, &cfg) != SIMMR_OK) return ev.fail("--eval-corrected");
  if (int rc = add_pieces(ev, "--eval-corrected-truth", args.eval_corrected_truth, LINES, simmr_correval_truth_add, simmr_last_correval_ms)) return rc;
  uint64_t n_entries = 0;
  if (simmr_correval_truth_plan(ev.h, &n_entries) != SIMMR_OK) return ev.fail("--eval-corrected-truth");
  if (int rc = add_pieces(ev, "--eval-corrected", args.eval_corrected, PieceCut{PieceCut::Record, lpr}, simmr_correval_add, simmr_last_correval_ms)) return rc;
  simmr_correval_counts c{};
  static_assert(sizeof(c) == CORREVAL_N_COUNTS * sizeof(uint64_t), "the report names every count");
  static_assert(CORREVAL_N_QUALS == SIMMR_CORREVAL_QUALS && CORREVAL_N_POS == SIMMR_CORREVAL_POS, "the report's rows are the tables'");
  std::vector<uint64_t> cube(125), by_qual(CORREVAL_N_QUALS * 5), by_pos(CORREVAL_N_POS * 5);
  if (simmr_correval_read(ev.h, &c, cube.data(), by_qual.data(), by_pos.data()) != SIMMR_OK) return ev.fail("--eval-corrected");
  std::string rows;
  if (!args.eval_corrected_reads.empty()) {
    Columns cols;  // key; length, before, residual, hits
    if (int rc = cols.room("--eval-corrected-reads", 1, 4, n_entries)) return rc;
    if (simmr_correval_emit(ev.h, cols.dw(0), cols.du(0), cols.du(1), cols.du(2), cols.du(3), n_entries) != SIMMR_OK) return ev.fail("--eval-corrected-reads");
    if (int rc = cols.fetch("--eval-corrected-reads")) return rc;
    rows = correval_read_rows(cols.w(0), cols.u(0), cols.u(1), cols.u(2), cols.u(3), n_entries);
  }
  if (int rc = write_text("--eval-corrected-report", args.eval_corrected_report, correval_report((const uint64_t*)&c, cube.data(), by_qual.data(), by_pos.data()))) return rc;
  if (!args.eval_corrected_reads.empty())
    if (int rc = write_text("--eval-corrected-reads", args.eval_corrected_reads, rows)) return rc;
  info("Truth: " + n(c.truth_entries) + " reads (" + n(c.truth_skipped) + " records skipped)");
  info("Corrected: " + n(c.records) + " records, " + n(c.unknown_read) + " of unknown reads, " + n(c.trimmed_records) + " trimmed, " + n(c.longer_records) + " longer");
  info("Bases: " + n(c.kept) + " kept, " + n(c.damaged) + " damaged, " + n(c.fixed) + " fixed, " + n(c.left) + " left, " + n(c.miscorrected) + " miscorrected, " +
       n(c.trimmed_error) + " errors trimmed away");
  info("Reads: " + n(c.fixed_all) + " fixed, " + n(c.improved) + " improved, " + n(c.unchanged) + " unchanged, " + n(c.worse) + " worse, " + n(c.clean_damaged) +
       " clean ones damaged, " + n(c.missing) + " without a record");
  info("Wrote " + args.eval_corrected_report);
  return 0;
}
