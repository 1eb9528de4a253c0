// simmr_host.hpp — C++ host layer above the C ABI: the callers and data formats
// either side of the accelerated path, mirroring the reference's own modules
// (same names, argument meaning and error behaviour):
//   genome.rs   -> Seq, Genome, Genome::from_fasta
//   files.rs    -> GenomeRecord, parse_genome_file, write_metadata
//   fastq.rs    -> write_to_fastq (header template interpolation)
//   error_profiles/*.rs, abundance_profiles/*.rs -> ErrorProfile, AbundanceProfile
//   cli.rs      -> CliArgs, determine_error_profile, determine_abundance_profile
// No simulation arithmetic lives here: reads come from libsimmr_hip.so.
#pragma once
#include <cstdint>
#include <cstdio>
#include <memory>
#include <optional>
#include <functional>
#include <string>
#include <vector>

#include "../../include/simmr_hip.h"

namespace simmr_host {

// ---------------------------------------------------------------- genome.rs
struct Seq {  // genome.rs:17-23
  std::string id;    // FASTA header line (needletail record.id())
  uint64_t uuid = 0;
  std::string seq;   // normalised sequence
  uint64_t size = 0;
};

struct Genome {  // genome.rs:26-41
  std::string uuid;
  std::string filepath;
  std::vector<Seq> sequence;
  uint64_t size = 0;
  uint64_t num_seqs = 0;
  std::optional<double> abundance;
  bool contiguous = false;

  // genome.rs:89-162.  Returns an error string on failure (Result<Genome, String>).
  static bool from_fasta(const std::string& filepath, bool contiguous, Genome* out, std::string* err);
};

// The record structure of a FASTA file without its sequences: what Genome::from_fasta does before it
// normalises (genome.rs:93-112).  `data` is the file; record c has header ids[c] and the raw body
// data[body[c].first, body[c].first + body[c].second) — the input of simmr_stage_fasta, which normalises
// and packs on the device.
struct FastaRecords {
  std::string data;
  std::vector<std::string> ids;
  std::vector<std::pair<size_t, size_t>> body;
};
bool scan_fasta(const std::string& filepath, FastaRecords* out, std::string* err);

// needletail 0.4.1 Sequence::normalize(iupac = false) as used at genome.rs:114
std::string normalize(const std::string& raw);
// util.rs:124-129: first 64 bits of a random UUID v4
uint64_t generate_id();
std::string uuid_from_u64(uint64_t u);  // genome.rs:69-73: format!("{:x}", u)

// ---------------------------------------------------------------- files.rs
struct GenomeRecord {  // files.rs:19-26
  std::string filepath;
  std::optional<std::string> uuid;
  std::optional<double> abundance;
};
bool parse_genome_file(const std::string& filepath, std::vector<GenomeRecord>* out, std::string* err);
struct MetadataRow {
  std::string genome_id, filepath;
  uint64_t num_reads;
  double abundance;
};
// One output file, as every writer here uses it: opened once ("wb" replaces, "ab" appends), text appended through a 1 MiB
// buffer, closed once.  The open, every fwrite and the fclose end in one status, and the two messages are made here only:
// "cannot open <path>" and "short write to <path>".
class OutFile {
 public:
  OutFile(const std::string& path, bool append) : path_(path), f_(fopen(path.c_str(), append ? "ab" : "wb")) {
    if (!f_) error_ = "cannot open " + path_;
  }
  OutFile(const OutFile&) = delete;
  ~OutFile() { if (f_) fclose(f_); }  // (without a word, and the text still buffered is dropped: the way out of a writer that fails)
  bool ok() const { return error_.empty(); }
  const std::string& error() const { return error_; }
  void append(const void* p, size_t n) {
    if (n == 0) return;
    if (buf_.size() + n >= BUFFER) { write(buf_.data(), buf_.size()); buf_.clear(); }
    if (n >= BUFFER) write(p, n);  // (a block this large goes to the file as it is)
    else buf_.append((const char*)p, n);
  }
  void append(const std::string& s) { append(s.data(), s.size()); }
  bool close(std::string* err) {  // false with *err = error() if anything failed since the open
    write(buf_.data(), buf_.size()); buf_.clear();
    if (f_ && fclose(f_) != 0 && ok()) error_ = "short write to " + path_;
    f_ = nullptr;
    if (!ok()) *err = error_;
    return ok();
  }
 private:
  static constexpr size_t BUFFER = 1u << 20;
  void write(const void* p, size_t n) { if (f_ && ok() && n && fwrite(p, 1, n, f_) != n) error_ = "short write to " + path_; }
  std::string path_, error_, buf_;
  FILE* f_;
};
bool write_metadata(const std::vector<MetadataRow>& rows, const std::string& output, std::string* err);
// Rust `{}` for f64: shortest digits that round-trip, never scientific notation
std::string format_f64_display(double v);

// ---------------------------------------------------------------- fastq.rs
// Host copy of one shard's SoA (simmr_reads_out columns).
struct HostReads {
  uint64_t n_reads = 0;
  bool paired = false;
  std::vector<uint8_t> seq, qual;  // qual already +33 (qual_offset = 33)
  std::vector<uint64_t> seq_off, start, end;
  std::vector<uint32_t> contig, genome, read_id;
  std::vector<uint8_t> flags;
};
// header_format.replace(...) chain of fastq.rs:34-56 for one read
std::string format_header(const std::string& header_format, const std::string& genome_id, uint32_t read_id,
                          const std::string& sequence_id, uint64_t start, uint64_t end, bool revcomp,
                          int pair);
// fastq.rs:14-124 for reads [first, first+count) of `reads`, all from `genome`
bool write_to_fastq(const std::string& genome_uuid, const Genome& genome, const HostReads& reads,
                    uint64_t first, uint64_t count, const std::string& output,
                    const std::string& header_format, bool append, std::string* err);

// ---------------------------------------------------------------- ground truth per read (no reference counterpart)
// Host copy of simmr_truth_out for the reads of one HostReads.
struct HostTruth {
  std::vector<uint32_t> nm;
  std::vector<uint64_t> edit_off;
  std::vector<uint32_t> edit_pos;
  std::vector<uint8_t> edit_ref, edit_alt, edit_qual;  // edit_qual as stored (Phred + qual_offset)
};
// `simmr-hip --truth FILE`: one tab-separated line per read, in read order:
//   read_id  pair  genome_id  sequence_id  start  end  strand  length  NM  edits
// pair 1 / 2 (0 for long reads), strand '-' iff reverse-complemented, edits `*` or a comma-joined list of
// pos:REF>ALT:Q (Q the decimal Phred).  reads.genome[r] indexes `genomes`.  with_header: the line of column names
// first (simmr-hip writes it with no reads when the run starts; every range then appends its reads).  Appends to `output`.
bool write_truth_tsv(const std::vector<Genome>& genomes, const HostReads& reads, const HostTruth& truth, uint32_t qual_offset,
                     const std::string& output, bool with_header, std::string* err);

// ---------------------------------------------------------------- SAM (no reference counterpart)
// `simmr-hip --sam FILE`: the alignment lines come from the device (simmr_sam_plan / simmr_sam_emit); the host gives the names
// and writes the header.  RNAME of a sequence: the first whitespace-delimited token of its id.
std::string sam_rname(const std::string& sequence_id);
// SAM's [0-9A-Za-z!#$%&+./:;?@^_|~-][0-9A-Za-z!#$%&*+./:;=?@^_|~-]*, at most 254 bytes
bool sam_rname_legal(const std::string& rname);
// "@HD\tVN:1.6\tSO:unsorted", one "@SQ\tSN:..\tLN:.." per name in order, "@PG\tID:simmr-hip\tPN:simmr-hip".  false with *err naming
// the first name that is not legal or that an earlier one has already.
// `coordinate`: SO:coordinate, for the file of --sam-sorted.
bool sam_header_text(const std::vector<std::string>& rnames, const std::vector<uint64_t>& lengths, std::string* out, std::string* err,
                     bool coordinate = false);
// `simmr-hip --eval-sam`: the SN: values of the @SQ lines of `text` (whole lines; the last may lack its newline), appended to
// *names in file order.  An @SQ line without an SN: field gives nothing.
void mapeval_sq_names(const char* text, size_t n, std::vector<std::string>* names);
// The file of --eval-report, in the shape of paftools mapeval: the counts of struct simmr_mapeval_counts as "#name\tvalue" lines in
// the struct's order (counts[MAPEVAL_N_COUNTS]), then from MAPQ 255 downwards one row per MAPQ that has mapped records:
// Q, the MAPQ, mapped at it, wrong at it, cumulative wrong / cumulative mapped (%.6g), cumulative mapped.  by_mapq[q * 2] counts
// the correct and by_mapq[q * 2 + 1] the wrong records of MAPQ q.
constexpr size_t MAPEVAL_N_COUNTS = 19;
std::string mapeval_report(const uint64_t* counts, const uint64_t* by_mapq);
// The rows of --eval-reads for n truth entries in key order: id, mate bit, class (0 no record, 1 unmapped, 2 wrong), MAPQ and
// records of every entry whose best class is not 3, tab-separated.
std::string mapeval_read_rows(const uint64_t* key, const uint32_t* best, const uint32_t* hits, size_t n);
// The file of --eval-overlaps-report: the counts of struct simmr_ovleval_counts as "#name\tvalue" lines in the struct's order
// (counts[OVLEVAL_N_COUNTS]); "#sensitivity" = pairs_found / truth_entries and "#precision" = correct / (correct + wrong), with six
// decimals, "0" where the denominator is 0; then a row per bit length with an entry in by_len[OVLEVAL_LEN_ROWS][2]: L, the bit
// length of the true overlap, the pairs found, the pairs not found.
constexpr size_t OVLEVAL_N_COUNTS = 16, OVLEVAL_LEN_ROWS = 41;
std::string ovleval_report(const uint64_t* counts, const uint64_t* by_len);
// The rows of --eval-overlaps-pairs for n truth entries in pair order: the two read names rebuilt from the keys (the id, and
// "/2" where the mate bit is set: a key does not keep whether a name of mate 0 carried "/1"), ov, best (0 no record, 2 wrong,
// 3 correct) and records, tab-separated.
std::string ovleval_pair_rows(const uint64_t* key_a, const uint64_t* key_b, const uint64_t* ov, const uint32_t* best, const uint32_t* hits, size_t n);
// The contig names of a VCF header: the ID of every "##contig=<ID=NAME[,...]>" line of text[0, n), in file order.
void vcfeval_contig_names(const char* text, size_t n, std::vector<std::string>* names);
// The file of --eval-vcf-report: the counts of struct simmr_vcfeval_counts as "#name\tvalue" lines in the struct's order
// (counts[VCFEVAL_N_COUNTS]); "#precision" = correct / calls and "#recall" = sites_found / truth_entries, each as the exact
// fraction "num/den" and, behind a tab, as a percentage with four decimals ("0" where the denominator is 0); then from QUAL row 255
// downward a row per row of by_qual[256][2] with a call: Q, the row, correct, wrong, and cumulatively over the rows so far the
// precision (correct / calls) and the correct calls per truth entry, each as fraction and percentage — the latter is the recall at
// that threshold where no site is called more than once (sites_multiple is 0), and an upper bound of it otherwise; then a row per
// row of by_ad[VCFEVAL_AD_ROWS][2] with an entry: AD, the bit length of ad_alt, the sites found, the sites not found.
constexpr size_t VCFEVAL_N_COUNTS = 24, VCFEVAL_AD_ROWS = 33;
std::string vcfeval_report(const uint64_t* counts, const uint64_t* by_qual, const uint64_t* by_ad);
// The rows of --eval-vcf-sites for n truth entries in key order: the contig name (names: the sorted names, the row is key >> 40),
// the 1-based position, ref, alt, ad_alt, the class of the best call (0 none, 2 wrong, 3 correct), its QUAL row and the calls,
// tab-separated.  A row whose name index is outside `names` gets "?".
std::string vcfeval_site_rows(const std::vector<std::string>& names, const uint64_t* key, const uint32_t* alleles, const uint32_t* ad, const uint32_t* best,
                              const uint32_t* hits, size_t n);
// ---- --eval-classified: the host's share (the files that are small, and the three texts) ----
constexpr size_t TAXEVAL_N_COUNTS = 13, TAXEVAL_RANKS = 8, TAXEVAL_CLASSES = 5;
// The rank code of a rank's name as NCBI's nodes.dmp spells it: 1 domain or superkingdom, 2 phylum, 3 class, 4 order, 5 family,
// 6 genus, 7 species, 8 strain; 0 any other text.  ... and the name a code is written with ("no_rank" for 0).
uint8_t taxeval_rank_code(const std::string& name);
const char* taxeval_rank_name(uint32_t code);
// The nodes of --eval-taxonomy from text[0, n): a line is "taxid | parent | rank | ..." with the separator "<tab>|<tab>" (NCBI's
// nodes.dmp; a "<tab>|" that ends the line is dropped) or "taxid <tab> parent <tab> rank"; the first three fields are read, empty
// lines are skipped.  false, and the line's number in *err: a line without three fields, or a taxid or parent that is no number
// of 1 to 10 digits below 2^32.
bool taxeval_parse_nodes(const char* text, size_t n, std::vector<uint32_t>* taxid, std::vector<uint32_t>* parent, std::vector<uint8_t>* rank, std::string* err);
// The map of --eval-genome-taxa from text[0, n): "genome_id <tab> taxid" a line; a first line whose second field is no number is a
// header; empty lines are skipped.  false, and the line's number in *err: a line without two fields, or a taxid that is no such number.
bool taxeval_parse_map(const char* text, size_t n, std::vector<std::string>* genome_id, std::vector<uint32_t>* taxid, std::string* err);
// The file of --eval-classified-report: the counts of struct simmr_taxeval_counts as "#name\tvalue" lines in the struct's order
// (counts[TAXEVAL_N_COUNTS]); an R row per rank with by_rank[8][5] and reads_by_rank[8][5] (absent, unclassified, wrong, above,
// correct); a P row per rank with precision = correct / (correct + wrong), sensitivity = correct / (unclassified + wrong + above +
// correct) and F1 = 2 P S / (P + S), on the records and then on the reads, "%.6f", "NA" where a denominator is 0; an A row per rank
// with the nodes of that rank and the L1 distance between the true and the called relative abundances over them, from the clade
// sums (rank_code, true_sum, called_sum: n_nodes entries in taxid order), each side normalised by its own sum at that rank, "NA"
// where either sum is 0.  Each block has a header line that starts with '#'.
std::string taxeval_report(const uint64_t* counts, const uint64_t* by_rank, const uint64_t* reads_by_rank, const uint8_t* rank_code, const uint64_t* true_sum,
                           const uint64_t* called_sum, size_t n_nodes);
// The rows of --eval-classified-reads for n truth entries in id order: the read id, the genome id (genome_ids: sorted, the row is
// its index; "?" outside), the lines behind the entry, its records, and the best class at each of the 8 ranks: the highest set bit
// of the rank's nibble of seen, plus one; for an entry without a record 1 where the genome's lineage has the rank (genome_has[row]
// bit r - 1) and 0 where not.
std::string taxeval_read_rows(const std::vector<std::string>& genome_ids, const std::vector<uint32_t>& genome_has, const uint64_t* id, const uint32_t* genome,
                              const uint32_t* mates, const uint32_t* seen, const uint32_t* hits, size_t n);
// The rows of --eval-classified-taxa: for every node (taxid order) with a clade sum that is not zero its taxid, the name of its rank,
// true, called, both, precision = both / called and recall = both / true ("%.6f", or "NA").
std::string taxeval_taxa_rows(const uint32_t* taxid, const uint8_t* rank_code, const uint64_t* true_sum, const uint64_t* called_sum, const uint64_t* both_sum,
                              size_t n_nodes);
// ---- --eval-assembly: the host's share (the names of the records, the contiguity, the two files) ----
constexpr size_t ASMEVAL_N_COUNTS = 18, ASMEVAL_GENOME_COLS = 5;
// The records of the FASTA text[0, n), which begins at a line's start: per header line (a '>' that begins a line) its first word
// (the text behind '>' up to a blank, a tab, a '\r' or the line's end) and the bytes of the record's sequence lines without their line
// ends (a '\r' directly before '\n' is part of the line end).  Sequence lines in front of the first header are not counted.
void asmeval_fasta_records(const char* text, size_t n, std::vector<std::string>* first_word, std::vector<uint64_t>* length);
// (records, bases, the longest record, N50: the length of the record at which the lengths, longest first, reach half the bases)
void asmeval_contiguity(const uint64_t* length, size_t n, uint64_t out[4]);
// The file of --eval-assembly-report: the counts of struct simmr_asmeval_counts as "#name\tvalue" lines in the struct's order
// (counts[ASMEVAL_N_COUNTS]); "#k"; "#completeness" = the entries with a hit / the entries, as the exact fraction and "%.6f" ("NA"
// without entries); "#qv" = -10 log10(1 - (1 - novel / kmers)^(1/k)) as "%.4f", "inf" where novel is 0, "NA" without k-mers;
// "#truth_contiguity" and "#contigs_contiguity" with records, bases, longest and N50; then a header line and a G row per genome
// (genomes: the sorted names) and one for "shared" with the five columns of by_genome[n + 1][5] and distinct_found / distinct.
std::string asmeval_report(const uint64_t* counts, uint32_t k, const std::vector<std::string>& genomes, const uint64_t* by_genome, const uint64_t* truth_length,
                           size_t n_truth, const uint64_t* contig_length, size_t n_contigs);
// The rows of --eval-assembly-contigs for n contigs in row order: the name (names[i]; "?" beyond them), length, kmers, found, shared,
// top_genome, top_kmers, and the genome's name (genomes: sorted, the row is its index), "." where the contig has no vote.
std::string asmeval_contig_rows(const std::vector<std::string>& names, const std::vector<std::string>& genomes, const uint64_t* length, const uint32_t* kmers,
                                const uint32_t* found, const uint32_t* shared, const uint32_t* top_genome, const uint32_t* top_kmers, size_t n);
// ---- --eval-placement: the host's share (the names come from asmeval_fasta_records; NA50 / NGA50 and the three files) ----
constexpr size_t ASMMAP_N_COUNTS = 27, ASMMAP_GENOME_COLS = 5, ASMMAP_BLOCK_COLS = 9;
// The length of the block at which the lengths, longest first, reach half of `target`, as a decimal number; "NA" where they never
// do (NA50: the target is the contigs' bases; NGA50: the truth's).
std::string asmmap_nga50(const uint64_t* block_length, size_t n, uint64_t target);
// The file of --eval-placement-report: the counts of struct simmr_asmmap_counts as "#name\tvalue" lines in the struct's order
// (counts[ASMMAP_N_COUNTS]); "#k", "#band", "#relocation", "#min_anchors"; "#misassemblies" = the four non-local classes; "#NA50" and
// "#NGA50" over the block lengths (block_length[n_blocks] = q_end - q_start; "NA" too where the target is 0); then a header line and
// a G row per genome (genomes: the sorted names) with the five columns of by_genome[n][5], the genome's own NGA50 (the blocks whose
// block_genome is the row, against half of its truth_bases) and block_bases / truth_bases as "%.6f" ("NA" without truth bases).
std::string asmmap_report(const uint64_t* counts, uint32_t k, uint32_t band, uint32_t relocation, uint32_t min_anchors, const std::vector<std::string>& genomes,
                          const uint64_t* by_genome, const uint64_t* block_length, const uint32_t* block_genome, size_t n_blocks);
// The rows of --eval-placement-blocks for n blocks in row order (cols: the nine columns of simmr_asmmap_blocks): the contig's name
// (contig_names[contig]; "?" beyond them), q_start, q_end, the truth record's first word (truth_names[truth_record]; "?" beyond
// them), p_start, p_end, '+' or '-', hits, and the join class by name (none, inter_genome, inter_record, inversion, relocation, local).
std::string asmmap_block_rows(const std::vector<std::string>& contig_names, const std::vector<std::string>& truth_names, const uint32_t* const cols[9], size_t n);
// The rows of --eval-placement-contigs for n contigs in row order: the name ("?" beyond the names), length, hits, blocks, first_block,
// block_bases and the worst join by name.
std::string asmmap_contig_rows(const std::vector<std::string>& names, const uint64_t* length, const uint32_t* hits, const uint32_t* blocks,
                               const uint32_t* first_block, const uint64_t* block_bases, const uint32_t* worst_join, size_t n);
// ---- --eval-corrected: the report and the reads file ----
// num / den to six decimals from the integers alone (millionths, rounded half up; '-' in front where `negative` and the result is
// not zero); "NA" where den is 0.
std::string correval_ratio(bool negative, uint64_t num, uint64_t den);
// The file of --eval-corrected-report: the counts of struct simmr_correval_counts as "#name\tvalue" lines in the struct's order
// (counts[CORREVAL_N_COUNTS]); "#gain" = (fixed - damaged) / (fixed + left + miscorrected + trimmed_error), "#sensitivity" = fixed / the
// same denominator and "#specificity" = kept / (kept + damaged), each as the exact fraction and correval_ratio; a header line and a Q
// row per quality that has a compared base (quality, kept, damaged, fixed, left, miscorrected: by_qual[q * 5 ..]); the same as P rows
// per position (by_pos); a header line and the cube's 25 C rows: the true base, the original base, and the corrected bases A C G T N
// (cube[(t * 5 + o) * 5 + c]).
constexpr size_t CORREVAL_N_COUNTS = 29, CORREVAL_N_QUALS = 95, CORREVAL_N_POS = 512;
std::string correval_report(const uint64_t* counts, const uint64_t* cube, const uint64_t* by_qual, const uint64_t* by_pos);
// The rows of --eval-corrected-reads for n truth entries in key order: id, mate bit, length, before, residual ('.' without a record)
// and records of every entry that has no record with residual 0, tab-separated.
std::string correval_read_rows(const uint64_t* key, const uint32_t* length, const uint32_t* before, const uint32_t* residual, const uint32_t* hits, size_t n);
// ---- --eval-bins: the host's share (the names of both texts, the report with its fractions, the two files) ----
constexpr size_t BINEVAL_N_COUNTS = 21, BINEVAL_GENOME_COLS = 7;
// The record lines of the truth text[0, n), which begins at a line's start (empty lines and lines that begin with '#' are none; a
// '\r' directly before '\n' is not part of the line): per line its field 1 and its field 8 ("" where the line has fewer fields).
void bineval_truth_names(const char* text, size_t n, std::vector<std::string>* contig, std::vector<std::string>* genome);
// The record lines of the candidate text[0, n) (lines that begin with '#' or '@' are none): per line its field 2 ("" without one).
void bineval_record_bins(const char* text, size_t n, std::vector<std::string>* bin);
// The adjusted Rand index of the assigned contigs of real genomes from the three pair sums and their number n, as "%.6f":
// (cells - E) / ((bins + genomes) / 2 - E) with E = bins * genomes / C(n, 2); "NA" where C(n, 2) or the denominator is 0.
std::string bineval_ari(uint64_t pairs_cells, uint64_t pairs_bins, uint64_t pairs_genomes, uint64_t n);
// The file of --eval-bins-report: the counts of struct simmr_bineval_counts as "#name\tvalue" lines in the struct's order
// (counts[BINEVAL_N_COUNTS]); "#purity" = sum_top_bases / assigned_bases and "#completeness" = sum_best_bases / the truth bases of the
// real genomes, each as the exact fraction and "%.6f" ("NA" where the denominator is 0); "#f1" of the two; "#assigned_fraction" =
// assigned_bases / truth_bases; "#ari_contigs" (bineval_ari with n = the assigned contigs of the real genomes); "#average_purity" =
// the mean over the bins with bases of top_bases / bases and "#average_completeness" = the mean over the real genomes with truth
// bases of best_bases / truth_bases, summed in row order in double; then a header line and a G row per genome (genomes: the sorted
// names; "." for the last row) with the seven columns of by_genome[n + 1][7] and best_bases / truth_bases, and a header line and a B
// row per bin: its name (bin_names[b]; "?" beyond them), contigs, bases, the top genome's name or ".", top_bases, none_bases,
// purity = top_bases / bases and completeness = top_bases / the truth bases of the top genome.
std::string bineval_report(const uint64_t* counts, const std::vector<std::string>& genomes, const uint64_t* by_genome, const std::vector<std::string>& bin_names,
                           const uint32_t* contigs, const uint64_t* bases, const uint64_t* none_bases, const uint32_t* top_genome, const uint64_t* top_bases,
                           size_t n_bins);
// The rows of --eval-bins-bins for n cells: the bin's name, the genome's name or ".", contigs, bases.
std::string bineval_cell_rows(const std::vector<std::string>& bin_names, const std::vector<std::string>& genomes, const uint32_t* bin, const uint32_t* genome,
                              const uint32_t* contigs, const uint64_t* bases, size_t n);
// The rows of --eval-bins-contigs for n truth contigs in truth order: name, length, the genome's name or ".", the bin's name or ".", records.
std::string bineval_contig_rows(const std::vector<std::string>& names, const std::vector<std::string>& genomes, const std::vector<std::string>& bin_names,
                                const uint32_t* genome, const uint64_t* length, const uint32_t* bin, const uint32_t* records, size_t n);
// ---- a file in pieces: what the nine commands that run no simulation read their files with ----
// Where a piece of a file that has not ended is cut: behind the last '\n' (Newline); in front of the last '>' that begins a line
// and is not the buffer's first byte (Fasta); behind the last '\n' whose number, counted from the buffer's start, is a multiple of
// `lines` (Record).
struct PieceCut {
  enum Kind { Newline, Fasta, Record } kind = Newline;
  uint32_t lines = 1;  // of a record (Record only)
};
// The cut of the buffer p[0, have) under `rule`; 0: the buffer holds no boundary, read on.
size_t piece_cut(const uint8_t* p, size_t have, PieceCut rule);
constexpr size_t FILE_PIECE = 64u << 20;  // bytes of one fread
// The pieces of a file: next() reads `piece_bytes` at a time until the buffer holds a cut, hands out the bytes in front of it and
// carries the rest over into the next piece; a line or record longer than a read makes the buffer grow.  At the end of the file the
// remainder is one piece, whether or not it ends in a newline.  No piece is longer than `max_bytes` (what one add takes): TooLong
// where a cut passes it, and under Fasta already where the buffer passes it with no cut in sight.
class PieceReader {
 public:
  enum End { Piece, Done, CannotRead, TooLong };
  PieceReader(FILE* f, PieceCut rule, size_t max_bytes, size_t piece_bytes = FILE_PIECE) : f_(f), rule_(rule), max_(max_bytes), piece_(piece_bytes) {}
  // Piece: p[0, n) is the next piece, good until the next call; any other answer is the walk's end
  End next(const uint8_t** p, size_t* n);

 private:
  FILE* f_;
  PieceCut rule_;
  size_t max_, piece_;
  std::vector<uint8_t> buf_;
  size_t have_ = 0, cut_ = 0;  // bytes of buf_ read; of those, handed out by the last call
  bool eof_ = false;
};
// `simmr-hip --sam FILE --sam-sorted` over several ranges: every range's lines come sorted from the device
// (simmr_sam_sort_plan / simmr_sam_sort_emit) with the key and the length of each.  A run is one range's lines: its keys
// ascend, and its text lies at `offset` of the byte source.
struct SamSortedRun {
  std::vector<uint64_t> key;  // of every line, ascending
  std::vector<uint64_t> len;  // bytes of every line
  uint64_t offset = 0;        // of the run's first byte in the source
};
// The k-way merge: the lines of every run in the order of (key, run number, position in the run) — which makes the output the
// stable sort of the runs' lines laid end to end.  read(offset, n, dst) fetches n bytes of the source, write(p, n) takes the
// merged bytes in order; either may answer false, and the merge then ends with false.
bool sam_merge_sorted_runs(const std::vector<SamSortedRun>& runs, const std::function<bool(uint64_t, size_t, char*)>& read,
                           const std::function<bool(const char*, size_t)>& write);
// Where the sorted runs of --sam-sorted and --bam-sorted wait for the merge.  The first run's bytes stay in memory: a run of one
// range needs no file.  From the second run on the runs lie back to back in the temporary file `<out>.sorting.tmp` (each run's
// `offset` is its place there).  merge() hands the one run as it is, or the runs merged by (key, run, place in the run), to the
// sink; the file goes there and on every other way out.
class SortedRunSpill {
 public:
  explicit SortedRunSpill(const std::string& out) : tmp_(out + ".sorting.tmp") {}
  SortedRunSpill(const SortedRunSpill&) = delete;
  ~SortedRunSpill() { drop(); }
  const std::vector<SamSortedRun>& runs() const { return runs_; }
  bool spilled() const { return on_disk_; }
  // run: the keys and lengths of `bytes`, which are the run's lines or records back to back
  bool add(SamSortedRun run, std::vector<uint8_t> bytes, std::string* err) {
    if (runs_.empty()) {
      first_ = std::move(bytes);
      runs_.push_back(std::move(run));
      return true;
    }
    if (!on_disk_) {
      on_disk_ = true;
      if (!write(first_, false, err)) return false;
      std::vector<uint8_t>().swap(first_);
    }
    run.offset = tmp_bytes_;
    if (!write(bytes, true, err)) return false;
    runs_.push_back(std::move(run));
    return true;
  }
  // false with *err untouched: the sink refused the one run; false with *err set: the file or the merge failed
  bool merge(const std::function<bool(const char*, size_t)>& sink, std::string* err) {
    if (!on_disk_) return first_.empty() || sink((const char*)first_.data(), first_.size());
    FILE* src = fopen(tmp_.c_str(), "rb");
    if (!src) { *err = "cannot open " + tmp_; drop(); return false; }
    const bool merged = sam_merge_sorted_runs(
        runs_, [&](uint64_t at, size_t n, char* p) { return fseeko(src, (off_t)at, SEEK_SET) == 0 && fread(p, 1, n, src) == n; }, sink);
    fclose(src);
    drop();
    if (!merged) *err = "the merge of the sorted ranges failed";
    return merged;
  }

 private:
  bool write(const std::vector<uint8_t>& bytes, bool append, std::string* err) {
    OutFile f(tmp_, append);
    f.append(bytes.data(), bytes.size());
    if (!f.close(err)) return false;
    tmp_bytes_ += bytes.size();
    return true;
  }
  void drop() { if (on_disk_) remove(tmp_.c_str()); }
  std::string tmp_;
  std::vector<SamSortedRun> runs_;
  std::vector<uint8_t> first_;
  uint64_t tmp_bytes_ = 0;
  bool on_disk_ = false;
};

// `simmr-hip --bam FILE --bam-sorted`: the merged stream (header and records) goes to the framing in pieces of a whole number
// of BGZF blocks (65 280 source bytes each); what does not fill a piece is carried into the next, so only the file's last block
// is short and the virtual offset of an uncompressed position is arithmetic (simmr_bai_plan's contract).  frame(p, n) takes a
// piece: n is piece_blocks * 65280 for every call but the last one, which finish() makes with what is left (none if nothing is).
class BgzfPieces {
 public:
  static constexpr size_t BLOCK = 65280;
  BgzfPieces(size_t piece_blocks, std::function<bool(const uint8_t*, size_t)> frame)
      : piece_((piece_blocks ? piece_blocks : 1) * BLOCK), frame_(std::move(frame)) { buf_.reserve(piece_); }
  bool append(const void* src, size_t n) {
    const uint8_t* p = (const uint8_t*)src;
    while (n > 0) {
      const size_t take = n < piece_ - buf_.size() ? n : piece_ - buf_.size();
      buf_.insert(buf_.end(), p, p + take);
      p += take; n -= take; bytes_ += take;
      if (buf_.size() == piece_) {
        if (!frame_(buf_.data(), buf_.size())) return false;
        buf_.clear();
      }
    }
    return true;
  }
  bool finish() {
    const bool ok = buf_.empty() || frame_(buf_.data(), buf_.size());
    buf_.clear();
    return ok;
  }
  uint64_t bytes() const { return bytes_; }  // appended so far

 private:
  size_t piece_;
  std::function<bool(const uint8_t*, size_t)> frame_;
  std::vector<uint8_t> buf_;
  uint64_t bytes_ = 0;
};

// ---------------------------------------------------------------- strain sites (no reference counterpart)
// Host copy of simmr_strain_out for one genome.
struct HostStrainSites {
  std::vector<uint32_t> contig;
  std::vector<uint64_t> pos;
  std::vector<uint8_t> ref, alt;
};
// `simmr-hip --strain-sites FILE`: a line of column names, then one tab-separated line per site of `genome`, in the order
// of the columns (sequence, then position):
//   genome_id  sequence_id  position  ref  alt
// position 0-based inside the sequence; the ids are the ones the FASTQ headers use.  with_header: the line of column names
// first (simmr-hip writes it with the run's first genome; every further genome appends its sites).  Appends to `output`.
bool write_strain_sites_tsv(const Genome& genome, const HostStrainSites& sites, const std::string& output, bool with_header,
                            std::string* err);

// `simmr-hip --strain-vcf FILE`: VCF 4.2 — ##fileformat, ##source=simmr-hip, one ##contig=<ID={genome_id}|{sequence_id},length=N>
// per sequence of the run (the naming of --gold-assembly; contig_len[g][c] its length in Seq.seq coordinates), the ##INFO lines
// of DP, AD, ADF, ADR (Number=R) and OTH, the eight-column #CHROM line, then one record per site in list order:
//   CHROM  pos+1  .  REF  ALT  .  .  DP=..;AD=r,a;ADF=r,a;ADR=r,a;OTH=..
// `sites` holds the sites of every genome back to back, site_genome[i] indexing `genomes`; counts is simmr_pileup_read's table,
// ten entries per site ([strand][class]).  r and a are the counts of REF's and ALT's classes, DP all ten, OTH = DP - AD's two
// numbers.  No sample columns.  Replaces `output`.
bool write_strain_vcf(const std::vector<Genome>& genomes, const std::vector<std::vector<uint64_t>>& contig_len, const HostStrainSites& sites,
                      const std::vector<uint32_t>& site_genome, const std::vector<uint32_t>& counts, const std::string& output,
                      std::string* err);

// ---------------------------------------------------------------- run statistics (no reference counterpart)
// `simmr-hip --stats FILE`: the tables of a simmr_run_stats (include/simmr_hip.h) in long form, tab-separated:
//   table  set  i  j  count
// one line per NON-ZERO entry, tables and entries in the struct's order; `set`, `i`, `j` are `-` where a table has no such
// index (reads, bases, cycle_n, cycle_qsum, cycle_mismatch: set and i; cycle_base: set, i = offset, j = class; pair: i =
// expected class, j = written class; the histograms and quality tables: i).  Replaces `output`.
bool write_stats_tsv(const simmr_run_stats& st, const std::string& output, std::string* err);
// `simmr-hip --fit-model FILE`: the model simmr_fit_plan made as the bincode image of a shared::encoding::ErrorModelParams, what
// `simmrd generate` writes and --custom-profile reads.  `cols` holds the columns of simmr_fit_emit copied to HOST memory (every
// one of kmer_ref, kmer_first, pair_alt, pair_prob, qual_density and the length / insert density, lo and hi columns that `info`
// gives a size); per position 71 densities beside num_bins 70 and ranges (i, i), bin_size 1.  The bytes are those of
// simmr_amd/model_io.py:serialize_fitted.  Replaces `output`.
std::string fit_model_bytes(const simmr_fit_info& info, const simmr_fit_out& cols);
bool write_fit_model(const simmr_fit_info& info, const simmr_fit_out& cols, const std::string& output, std::string* err);

// ---------------------------------------------------------------- coverage depth (no reference counterpart)
// `simmr-hip --depth FILE`: a line of column names, then one tab-separated line per contig, in the order of depth[]:
//   genome_id  sequence_id  length  covered  depth_sum  depth_max
// from the rows of simmr_depth_summarize; rows[k].genome indexes `genomes`.  Every column is an integer.  Replaces `output`.
bool write_depth_tsv(const std::vector<Genome>& genomes, const simmr_depth_contig* rows, uint64_t n_rows, const std::string& output,
                     std::string* err);
// `simmr-hip --depth-track FILE`: a line of column names, then one line per window of `window` positions:
//   genome_id  sequence_id  start  end  depth_sum  covered  depth_max
// start / end 0-based and half-open inside the sequence (a sequence's last window is partial); win_* are HOST copies of the
// columns of simmr_depth_windows, rows[k].first_window the index of contig k's first window.  Replaces `output`.
bool write_depth_track_tsv(const std::vector<Genome>& genomes, const simmr_depth_contig* rows, uint64_t n_rows, uint32_t window,
                           const uint64_t* win_sum, const uint32_t* win_covered, const uint32_t* win_max, const std::string& output,
                           std::string* err);

// ---------------------------------------------------------------- gold-standard assembly (no reference counterpart)
// Host copy of simmr_regions_out: one entry per region (seq_off one more), seq the regions' bases back to back.
struct HostRegions {
  std::vector<uint32_t> genome, contig;
  std::vector<uint64_t> start, len, depth_sum, seq_off;
  std::vector<uint8_t> seq;
};
// `simmr-hip --gold-assembly FILE`: one FASTA record per region, in the order of the columns:
//   >{genome_id}|{sequence_id}:{start+1}-{start+len} depth_sum={depth_sum}
// (1-based, closed coordinates inside the sequence) and the region's bases in lines of 80.  regions.genome[k] indexes
// `genomes`.  Replaces `output`.
bool write_gold_fasta(const std::vector<Genome>& genomes, const HostRegions& regions, const std::string& output, std::string* err);
// `simmr-hip --gold-regions FILE`: a line of column names, then one tab-separated line per region:
//   genome_id  sequence_id  start  length  depth_sum  seq_off
// start 0-based inside the sequence, seq_off the region's first base in the base stream.  regions.seq is not read.  Replaces `output`.
bool write_gold_regions_tsv(const std::vector<Genome>& genomes, const HostRegions& regions, const std::string& output, std::string* err);

// ------------------------------------------------------- error_profiles/*.rs
class ErrorProfile {  // error_profiles/base.rs:6-32 (the per-read methods run on the device)
 public:
  virtual ~ErrorProfile() = default;
  // extensions of the long-read kinds (--per-read-lengths / --uniform-start), read by their pod()
  uint32_t length_mode = SIMMR_LEN_REFERENCE;
  uint8_t long_start_mode = SIMMR_START_REFERENCE;
  virtual simmr_error_profile pod() const = 0;
  virtual uint16_t minimum_genome_size() const = 0;
  virtual bool is_long_read() const = 0;
};
struct PerfectShortErrorProfile : ErrorProfile {  // perfect_short.rs
  uint16_t read_length = 150, insert_size = 150;
  simmr_error_profile pod() const override;
  uint16_t minimum_genome_size() const override { return (uint16_t)(2u * read_length + insert_size); }
  bool is_long_read() const override { return false; }
};
struct MinimalShortErrorProfile : ErrorProfile {  // minimal_short.rs
  uint16_t read_length = 150, insert_size = 150;
  uint8_t mean_phred_score = 30;
  double insert_size_std = 75.0, read_length_std = 15.0;
  simmr_error_profile pod() const override;
  uint16_t minimum_genome_size() const override { return (uint16_t)(2u * read_length + insert_size); }
  bool is_long_read() const override { return false; }
};
struct MinimalLongErrorProfile : ErrorProfile {  // minimal_long.rs
  uint8_t mean_phred_score = 30;
  uint16_t read_length = 20000;  // unused by the reference (minimal_long.rs:64-65 hard-codes the gamma)
  double read_length_std = 5000.0;
  float gamma_mean = 20000.0f, gamma_std = 15000.0f;
  simmr_error_profile pod() const override;
  uint16_t minimum_genome_size() const override { return 20000; }
  bool is_long_read() const override { return true; }
};
struct PerfectLongErrorProfile : MinimalLongErrorProfile {  // perfect_long.rs
  simmr_error_profile pod() const override;
};

struct CustomShortErrorProfile : ErrorProfile {  // custom_short.rs (model read by cli.rs:255-272)
  std::vector<uint8_t> model;  // bincode ErrorModelParams, handed to the library as is
  double read_length_mean = 0, insert_size_mean = 0;
  bool is_long = false;
  // shared/src/encoding.rs:268-281 deserialize_model_from_path
  static std::unique_ptr<CustomShortErrorProfile> from_path(const std::string& path, std::string* err);
  simmr_error_profile pod() const override;
  uint16_t minimum_genome_size() const override;  // custom_short.rs:535-538
  bool is_long_read() const override { return is_long; }
};

// --------------------------------------------------- abundance_profiles/*.rs
using Abundances = std::vector<std::pair<uint64_t, double>>;
class AbundanceProfile {  // abundance_profiles/base.rs:10-69
 public:
  virtual ~AbundanceProfile() = default;
  virtual bool is_size_aware() const = 0;
  virtual Abundances determine_abundances(uint64_t total_reads, uint64_t num_genomes) const = 0;
  virtual Abundances adjust_for_size(const std::vector<Genome>& genomes, const Abundances& read_abundances,
                                     uint64_t read_length, bool paired) const;
};
struct UniformAbundanceProfile : AbundanceProfile {  // uniform.rs
  bool size_adjusted = false;
  bool is_size_aware() const override { return size_adjusted; }
  Abundances determine_abundances(uint64_t total_reads, uint64_t num_genomes) const override;
};
struct ExactAbundanceProfile : AbundanceProfile {  // exact.rs
  bool is_size_aware() const override { return false; }
  Abundances determine_abundances(uint64_t total_reads, uint64_t num_genomes) const override;
  Abundances adjust_for_size(const std::vector<Genome>&, const Abundances& a, uint64_t, bool) const override { return a; }
};
struct CustomAbundanceProfile : AbundanceProfile {  // custom.rs
  bool size_adjusted = false;
  std::vector<double> abundances;
  bool is_size_aware() const override { return size_adjusted; }
  Abundances determine_abundances(uint64_t total_reads, uint64_t num_genomes) const override;
};

// ---------------------------------------------------------------- cli.rs
enum class ErrorProfileKind { MinimalShort, MinimalLong, PerfectShort, PerfectLong, CustomShort, CustomLong /* extension */ };
enum class AbundanceProfileKind { Exact, Uniform, Custom };
struct CliArgs {  // cli.rs:93-220, same flags and defaults
  std::vector<std::string> genome;
  std::optional<std::string> genome_file;
  std::string output;
  uint64_t num_reads = 1000;
  uint16_t read_length = 150;
  double read_length_std = 10.0;
  uint16_t insert_size = 150;
  uint8_t mean_phred_score = 30;
  ErrorProfileKind error_profile = ErrorProfileKind::PerfectShort;
  AbundanceProfileKind abundance_profile = AbundanceProfileKind::Uniform;
  std::optional<std::string> custom_profile;
  std::optional<double> with_ani;  // a percentage, 25 .. 100 (decimals accepted): every genome of the run becomes a strain of that identity
  std::string read_header_format =
      "@{:read_id:}|{:genome_id:}/{:pair:} metadata:sid={:sequence_id:}|sp={:start_position:}|ep={:end_position:}|rc={:reverse_complement:}";
  std::optional<uint64_t> seed;
  bool size_adjusted = false;
  bool contiguous = false;
  // extensions of this implementation (not reference flags)
  int device = 0;
  std::vector<int> devices;  // --devices a,b,...: one engine per entry (an ordinal may repeat), the run's ranges dealt to them in turn
  bool host_normalize = false;  // --host-normalize: normalise FASTA on the host instead of the device
  bool host_fastq = false;  // --host-fastq: frame the FASTQ on the host instead of the device
  std::string truth;  // --truth FILE: per-read mismatch counts and edit lists (simmr_truth_plan / simmr_truth_emit) as a TSV
  bool sam_sorted = false;  // --sam-sorted: the file of --sam in coordinate order (simmr_sam_sort_plan / simmr_sam_sort_emit, a merge of the ranges)
  std::string sam;    // --sam FILE: the true alignments as SAM (simmr_sam_plan / simmr_sam_emit on every range's columns, the header from the host)
  std::string bam;    // --bam FILE: the same alignments as BAM in read order (simmr_bam_plan / simmr_bam_emit on every range's columns, framed by simmr_bgzf_frame: stored blocks; the header from the host)
  bool bam_sorted = false;  // --bam-sorted: the file of --bam in coordinate order with its BAI index (simmr_bam_sort_*, a merge of the ranges, simmr_bai_*)
  std::string bam_index;    // --bam-index FILE: where the index goes [default: the file of --bam with ".bai" appended]
  std::string overlaps;       // --overlaps FILE: the true read-to-read overlaps of the run as PAF (simmr_overlap_add over every range, one plan, drained by windows)
  uint64_t min_overlap = 1;   // --min-overlap N: shared reference bases from which two reads overlap
  std::string fit_model;      // --fit-model FILE: an error model fitted from the run (simmr_fit_add over every range, one plan) as simmrd writes it
  uint32_t fit_k = 7;         // --fit-k K: its k-mer size, 3 .. 10
  uint32_t fit_max_alt = 20;  // --fit-max-alt N: alternates kept per reference k-mer
  std::string fit_from_sam;   // --fit-from-sam FILE: no simulation; the model of --fit-model from the records of a SAM file (simmr_fit_add_sam)
  bool single_reads = false;  // --single-reads: with --fit-from-sam, the file holds unpaired reads (n_sets 1: no insert sizes)
  std::string eval_sam;       // --eval-sam FILE: no simulation; an aligner's SAM scored against the truth of --eval-truth (simmr_mapeval_*)
  std::string eval_truth;     // --eval-truth FILE: the true alignments (the file of --sam); its @SQ lines give the reference names
  std::string eval_report;    // --eval-report FILE: the counts and the rows by MAPQ as a TSV
  std::string eval_reads;     // --eval-reads FILE: every truth read whose best record is not correct
  uint32_t eval_min_overlap = 0;  // --eval-min-overlap PCT: 1 .. 100 (0: not given, the library's default of 10)
  std::string eval_overlaps;         // --eval-overlaps FILE: no simulation; an overlapper's PAF scored against the truth of --eval-overlaps-truth (simmr_ovleval_*)
  std::string eval_overlaps_truth;   // --eval-overlaps-truth FILE: the true overlaps (the file of --overlaps)
  std::string eval_overlaps_report;  // --eval-overlaps-report FILE: the counts, sensitivity, precision and the rows by overlap length as a TSV
  std::string eval_overlaps_pairs;   // --eval-overlaps-pairs FILE: a row per true pair
  uint32_t eval_overlaps_min_pct = 0;  // --eval-overlaps-min-pct PCT: 1 .. 100 (0: not given, the library's default of 10)
  std::string eval_vcf;         // --eval-vcf FILE: no simulation; a variant caller's VCF scored against the truth of --eval-vcf-truth (simmr_vcfeval_*)
  std::string eval_vcf_truth;   // --eval-vcf-truth FILE: the strain's sites (the file of --strain-vcf)
  std::string eval_vcf_report;  // --eval-vcf-report FILE: the counts, precision, recall, the rows by QUAL and by the alternate allele's reads as a TSV
  std::string eval_vcf_sites;   // --eval-vcf-sites FILE: a row per true site
  std::string eval_classified;         // --eval-classified FILE: no simulation; a read classifier's per-read output scored against --truth (simmr_taxeval_*)
  std::string eval_classified_truth;   // --eval-classified-truth FILE: the file of --truth
  std::string eval_taxonomy;           // --eval-taxonomy FILE: nodes.dmp, or taxid parent rank as a TSV
  std::string eval_genome_taxa;        // --eval-genome-taxa FILE: genome_id taxid as a TSV
  std::string eval_classified_report;  // --eval-classified-report FILE: the counts, a row per rank, precision / sensitivity / F1, the profile's L1 distance
  std::string eval_classified_reads;   // --eval-classified-reads FILE: a row per true read
  std::string eval_classified_taxa;    // --eval-classified-taxa FILE: a row per taxon with reads
  std::string eval_assembly;          // --eval-assembly FILE: no simulation; an assembler's contigs scored against --eval-assembly-truth (simmr_asmeval_*)
  std::string eval_assembly_truth;    // --eval-assembly-truth FILE: the file of --gold-assembly
  std::string eval_assembly_report;   // --eval-assembly-report FILE: the counts, completeness per genome and overall, the QV, the contiguity of both sides
  std::string eval_assembly_contigs;  // --eval-assembly-contigs FILE: a row per contig
  uint32_t eval_assembly_k = 31;      // --eval-assembly-k K: odd, 15 .. 31
  std::string eval_placement;          // --eval-placement FILE: no simulation; an assembler's contigs placed on --eval-placement-truth (simmr_asmmap_*)
  std::string eval_placement_truth;    // --eval-placement-truth FILE: the file of --gold-assembly
  std::string eval_placement_report;   // --eval-placement-report FILE: the counts, the misassemblies, NA50 / NGA50, a row per genome
  std::string eval_placement_blocks;   // --eval-placement-blocks FILE: a row per block
  std::string eval_placement_contigs;  // --eval-placement-contigs FILE: a row per contig
  uint32_t eval_placement_k = 31;      // --eval-placement-k K: odd, 15 .. 31
  uint32_t eval_placement_band = 64;          // --eval-placement-band N
  uint32_t eval_placement_relocation = 1000;  // --eval-placement-relocation N: below 2^31
  uint32_t eval_placement_min_anchors = 16;   // --eval-placement-min-anchors N: at least 1
  std::string eval_corrected;         // --eval-corrected FILE: no simulation; a corrector's FASTQ scored against --eval-corrected-truth (simmr_correval_*)
  std::string eval_corrected_truth;   // --eval-corrected-truth FILE: the file of --sam
  std::string eval_corrected_report;  // --eval-corrected-report FILE: the counts, gain, sensitivity, specificity, the rows by quality and position, the cube
  std::string eval_corrected_reads;   // --eval-corrected-reads FILE: a row per read that is not its true self
  bool eval_corrected_fasta = false;  // --eval-corrected-fasta: two-line FASTA records
  std::string eval_bins;              // --eval-bins FILE: no simulation; a binner's contig<TAB>bin text scored against --eval-bins-truth (simmr_bineval_*)
  std::string eval_bins_truth;        // --eval-bins-truth FILE: the file of --eval-assembly-contigs
  std::string eval_bins_report;       // --eval-bins-report FILE: the counts, purity, completeness, F1, ARI, a row per genome and per bin
  std::string eval_bins_bins;         // --eval-bins-bins FILE: the cells with names
  std::string eval_bins_contigs;      // --eval-bins-contigs FILE: a row per truth contig
  bool eval_vcf_filtered = false;  // --eval-vcf-filtered: score the records whose FILTER is neither "." nor PASS too
  std::string stats;  // --stats FILE: the run's quality, base and mismatch tables (simmr_stats_add over every range) as a TSV
  std::string depth;        // --depth FILE: covered positions, depth sum and maximum per contig (simmr_depth_add over every range) as a TSV
  std::string depth_track;  // --depth-track FILE: the same per window of --depth-window positions
  uint32_t depth_window = 1000;  // --depth-window W
  std::string gold_assembly;     // --gold-assembly FILE: the regions the run covered (simmr_regions_plan / simmr_regions_emit over the run's depth[]) as FASTA
  std::string gold_regions;      // --gold-regions FILE: the same regions' columns as a TSV
  uint32_t gold_min_depth = 1;   // --gold-min-depth D: a position belongs to a region from this depth on
  uint64_t gold_min_length = 1;  // --gold-min-length M: shorter runs are no regions
  std::string strain_sites;      // --strain-sites FILE: the sites --with-ani changed (simmr_strain_apply's columns) as a TSV
  std::string strain_vcf;        // --strain-vcf FILE: the same sites with the allele counts of the run's reads (simmr_pileup_add over every range) as VCF 4.2
  uint64_t device_chunk_reads = 0;  // --device-chunk-reads: reads generated per device pass (0: what fits the free device memory)
  std::optional<std::pair<float, float>> gamma;  // --gamma mean,std
  bool uniform_start = false;                    // --uniform-start (SIMMR_START_UNIFORM)
  bool per_read_lengths = false;                 // --per-read-lengths (SIMMR_LEN_PER_READ)
  bool rng_philox = false;  // --rng philox: the counter mode for the per-base draws (SIMMR_RNG_PHILOX; statistical parity,
                            // BASELINE.json north_star).  Default `reference`: the reference's own streams, byte-identical output
  bool rng_philox_full = false;  // --rng philox-full: the plan's draws from Philox counters too (SIMMR_RNG_PHILOX_FULL): minimal-short,
                                 // and minimal-long / perfect-long with --per-read-lengths
};
// returns false and fills err on a usage error (clap would exit(2)); help=true for --help
bool parse_cli_args(int argc, const char* const* argv, CliArgs* out, std::string* err, bool* help);
std::string usage();
std::unique_ptr<ErrorProfile> determine_error_profile(const CliArgs& args, std::string* err);   // cli.rs:229-301
std::unique_ptr<AbundanceProfile> determine_abundance_profile(const CliArgs& args,
                                                              std::optional<std::vector<double>> abundances);  // :306-320

}  // namespace simmr_host
