// host.cpp — implementation of simmr_host.hpp (no GPU code, no simulation
// arithmetic).  Each function cites the reference lines it mirrors.
#include "simmr_host.hpp"

#include "../csrc/custom_model.hpp"
#include "../csrc/fit_host.hpp"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <ctype.h>

#include <algorithm>
#include <fstream>
#include <queue>
#include <set>
#include <random>
#include <sstream>

namespace simmr_host {

// ------------------------------------------------------------------ genome.rs

std::string normalize(const std::string& raw) {
  // needletail 0.4.1 sequence::normalize(seq, iupac = false)
  std::string out;
  out.reserve(raw.size());
  for (unsigned char c : raw) {
    switch (c) {
      case 'A': case 'C': case 'G': case 'T': case 'N': case '-': out.push_back((char)c); break;
      case 'a': out.push_back('A'); break;
      case 'c': out.push_back('C'); break;
      case 'g': out.push_back('G'); break;
      case 't': case 'u': case 'U': out.push_back('T'); break;
      case '.': case '~': out.push_back('-'); break;
      case ' ': case '\t': case '\r': case '\n': break;  // whitespace and line endings are dropped
      default: out.push_back('N'); break;                // everything else is an N
    }
  }
  return out;
}

uint64_t generate_id() {
  // util.rs:124-129: Uuid::new_v4().as_u64_pair().0 — the version nibble (4) sits in bits 15..12
  static std::random_device rd;
  uint64_t r = ((uint64_t)rd() << 32) ^ (uint64_t)rd();
  return (r & ~0xF000ULL) | 0x4000ULL;
}

std::string uuid_from_u64(uint64_t u) {
  char buf[32];
  snprintf(buf, sizeof buf, "%llx", (unsigned long long)u);
  return buf;
}

bool scan_fasta(const std::string& filepath, FastaRecords* out, std::string* err) {
  std::ifstream f(filepath, std::ios::binary);
  if (!f) { *err = "No such file or directory (os error 2)"; return false; }
  std::stringstream ss;
  ss << f.rdbuf();
  out->data = ss.str();
  const std::string& data = out->data;
  if (data.empty()) { *err = "Failed to read the first two bytes. Is the file empty?"; return false; }
  if (data.size() >= 2 && (unsigned char)data[0] == 0x1f && (unsigned char)data[1] == 0x8b) {
    *err = "compressed FASTA is not supported by this host layer";
    return false;
  }
  if (data[0] != '>') { *err = "Bad starting byte found, expected '>' (FASTA records only)"; return false; }
  size_t pos = 0;
  while (pos < data.size()) {
    // header line
    size_t eol = data.find('\n', pos);
    if (eol == std::string::npos) eol = data.size();
    std::string header = data.substr(pos + 1, eol - pos - 1);
    if (!header.empty() && header.back() == '\r') header.pop_back();
    // sequence lines until a line starting with '>'
    size_t p = std::min(eol + 1, data.size());
    size_t next = p;
    for (;;) {
      if (next >= data.size()) { next = data.size(); break; }
      if (data[next] == '>') break;
      size_t e = data.find('\n', next);
      if (e == std::string::npos) { next = data.size(); break; }
      next = e + 1;
    }
    out->ids.push_back(header);                          // genome.rs:112 record.id()
    out->body.emplace_back(p, next - p);
    pos = next;
  }
  return true;
}

bool Genome::from_fasta(const std::string& filepath, bool contiguous, Genome* out, std::string* err) {
  FastaRecords recs;
  if (!scan_fasta(filepath, &recs, err)) return false;
  std::vector<Seq> sequences;
  for (size_t c = 0; c < recs.ids.size(); c++) {
    Seq s;
    s.id = recs.ids[c];
    s.uuid = generate_id();                              // genome.rs:118
    s.seq = normalize(recs.data.substr(recs.body[c].first, recs.body[c].second));  // genome.rs:114 normalize(false)
    s.size = s.seq.size();
    sequences.push_back(std::move(s));
  }
  Genome g;
  g.uuid = uuid_from_u64(generate_id());                 // genome.rs:124,140
  g.filepath = filepath;
  g.contiguous = contiguous;
  uint64_t total = 0;
  for (const Seq& s : sequences) total += s.seq.size();
  g.size = total;
  if (contiguous) {                                      // genome.rs:121-137
    Seq whole;
    whole.id = "whole genome";
    whole.uuid = generate_id();
    for (const Seq& s : sequences) { whole.seq += s.seq; whole.seq.push_back('N'); }
    whole.size = total;                                  // the 'N' separators are NOT counted
    g.sequence.push_back(std::move(whole));
    g.num_seqs = 1;
  } else {
    g.num_seqs = sequences.size();
    g.sequence = std::move(sequences);
  }
  *out = std::move(g);
  return true;
}

// ------------------------------------------------------------------- files.rs

static std::vector<std::string> split_tabs(const std::string& line) {
  std::vector<std::string> out;
  size_t a = 0;
  for (;;) {
    size_t b = line.find('\t', a);
    if (b == std::string::npos) { out.push_back(line.substr(a)); break; }
    out.push_back(line.substr(a, b - a));
    a = b + 1;
  }
  return out;
}

bool parse_genome_file(const std::string& filepath, std::vector<GenomeRecord>* out, std::string* err) {
  std::ifstream f(filepath);
  if (!f) { *err = "Genome file does not exist"; return false; }  // files.rs:57-59
  std::vector<std::string> lines;
  std::string line;
  while (std::getline(f, line)) {
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (!line.empty()) lines.push_back(line);
  }
  out->clear();
  if (lines.empty()) return true;
  // files.rs:32-45 decides "simple" only when the first line is at most one
  // character long, so every real file is read with a header row (csv crate,
  // tab delimiter; serde aliases path|filepath, id|genome_id|uuid).  A first line
  // that names no path column is accepted as a plain list (extension).
  std::vector<std::string> head = split_tabs(lines[0]);
  int c_path = -1, c_uuid = -1, c_ab = -1;
  for (size_t i = 0; i < head.size(); i++) {
    if (head[i] == "filepath" || head[i] == "path") c_path = (int)i;
    else if (head[i] == "uuid" || head[i] == "id" || head[i] == "genome_id") c_uuid = (int)i;
    else if (head[i] == "abundance") c_ab = (int)i;
  }
  size_t first_row = 1;
  if (c_path < 0) { c_path = 0; c_uuid = 1; c_ab = 2; first_row = 0; }  // positional, no header
  for (size_t r = first_row; r < lines.size(); r++) {
    std::vector<std::string> cols = split_tabs(lines[r]);
    GenomeRecord rec;
    if ((size_t)c_path >= cols.size()) { *err = "genome file row " + std::to_string(r + 1) + " has no path"; return false; }
    rec.filepath = cols[c_path];
    if (c_uuid >= 0 && (size_t)c_uuid < cols.size() && !cols[c_uuid].empty()) rec.uuid = cols[c_uuid];
    if (c_ab >= 0 && (size_t)c_ab < cols.size() && !cols[c_ab].empty()) {
      char* end = nullptr;
      double v = strtod(cols[c_ab].c_str(), &end);
      if (end == cols[c_ab].c_str() || *end != 0) { *err = "invalid abundance '" + cols[c_ab] + "'"; return false; }
      rec.abundance = v;
    }
    out->push_back(rec);
  }
  return true;
}

std::string format_f64_display(double v) {
  if (v != v) return "NaN";
  if (isinf(v)) return v < 0 ? "-inf" : "inf";
  if (v == 0) return signbit(v) ? "-0" : "0";
  char buf[64];
  int prec = 1;
  for (; prec <= 17; prec++) {
    snprintf(buf, sizeof buf, "%.*e", prec - 1, v);
    if (strtod(buf, nullptr) == v) break;
  }
  // buf = d.ddddde[+-]xx
  std::string s(buf);
  bool neg = s[0] == '-';
  if (neg) s.erase(0, 1);
  size_t epos = s.find('e');
  int exp10 = atoi(s.c_str() + epos + 1);
  std::string digits;
  for (size_t i = 0; i < epos; i++) if (s[i] != '.') digits.push_back(s[i]);
  while (digits.size() > 1 && digits.back() == '0') digits.pop_back();
  std::string out;
  int nd = (int)digits.size();
  if (exp10 >= nd - 1) {
    out = digits + std::string(exp10 - (nd - 1), '0');
  } else if (exp10 >= 0) {
    out = digits.substr(0, exp10 + 1) + "." + digits.substr(exp10 + 1);
  } else {
    out = "0." + std::string(-exp10 - 1, '0') + digits;
  }
  return neg ? "-" + out : out;
}

bool write_metadata(const std::vector<MetadataRow>& rows, const std::string& output, std::string* err) {
  // files.rs:100-134
  remove(output.c_str());
  OutFile out(output, false);
  out.append("genome_id\tfilepath\tnum_reads\tabundance\n");
  for (const MetadataRow& r : rows)
    out.append(r.genome_id + "\t" + r.filepath + "\t" + std::to_string(r.num_reads) + "\t" + format_f64_display(r.abundance) + "\n");
  return out.close(err);
}

// ------------------------------------------------------------------- fastq.rs

static void replace_all(std::string& s, const char* pat, const std::string& with) {
  const size_t n = strlen(pat);
  size_t pos = 0;
  while ((pos = s.find(pat, pos)) != std::string::npos) {
    s.replace(pos, n, with);
    pos += with.size();
  }
}

std::string format_header(const std::string& header_format, const std::string& genome_id, uint32_t read_id,
                          const std::string& sequence_id, uint64_t start, uint64_t end, bool revcomp,
                          int pair) {
  // the chained String::replace calls of fastq.rs:34-56, in the same order
  std::string h = header_format;
  replace_all(h, "{:genome_id:}", genome_id);
  replace_all(h, "{:read_id:}", std::to_string(read_id));
  replace_all(h, "{:sequence_id:}", sequence_id);
  replace_all(h, "{:start_position:}", std::to_string(start));
  replace_all(h, "{:end_position:}", std::to_string(end));
  replace_all(h, "{:reverse_complement:}", revcomp ? "t" : "f");
  replace_all(h, "{:pair:}", pair == 1 ? "1" : "2");
  return h;
}

bool write_to_fastq(const std::string& genome_uuid, const Genome& genome, const HostReads& reads,
                    uint64_t first, uint64_t count, const std::string& output,
                    const std::string& header_format, bool append, std::string* err) {
  OutFile out(output, append);
  for (uint64_t r = first; r < first + count; r++) {
    const uint64_t o = reads.seq_off[r];
    const bool rc = (reads.flags[r] & SIMMR_FLAG_REVCOMP) != 0;
    const uint64_t len = rc ? reads.start[r] - reads.end[r] : reads.end[r] - reads.start[r];
    // long reads are never pair 2; for pairs the mate is the parity of the read index
    const int pair = (reads.paired && (r & 1)) ? 2 : 1;
    const std::string& sid = genome.sequence[reads.contig[r]].id;
    std::string h = format_header(header_format, genome_uuid, reads.read_id[r], sid, reads.start[r],
                                  reads.end[r], rc, pair);
    h += '\n';
    out.append(h);
    out.append(reads.seq.data() + o, len);
    out.append("\n+\n", 3);
    out.append(reads.qual.data() + o, len);  // util::encode_quality_scores: +33, applied on the device
    out.append("\n", 1);
  }
  return out.close(err);
}

// --------------------------------------------------------------- SAM
std::string sam_rname(const std::string& id) {
  const char* ws = " \t\n\v\f\r";
  const size_t a = id.find_first_not_of(ws);
  if (a == std::string::npos) return "";
  const size_t b = id.find_first_of(ws, a);
  return id.substr(a, b == std::string::npos ? std::string::npos : b - a);
}
bool sam_rname_legal(const std::string& n) {
  if (n.empty() || n.size() > 254) return false;
  for (size_t i = 0; i < n.size(); i++) {
    const unsigned char c = (unsigned char)n[i];
    if (isalnum(c) || (c != 0 && strchr("!#$%&+./:;?@^_|~-", c))) continue;
    if (i > 0 && (c == '*' || c == '=')) continue;
    return false;
  }
  return true;
}
bool sam_header_text(const std::vector<std::string>& rnames, const std::vector<uint64_t>& lengths, std::string* out, std::string* err,
                     bool coordinate) {
  std::set<std::string> seen;
  *out = coordinate ? "@HD\tVN:1.6\tSO:coordinate\n" : "@HD\tVN:1.6\tSO:unsorted\n";
  for (size_t k = 0; k < rnames.size(); k++) {
    if (!sam_rname_legal(rnames[k])) { *err = "'" + rnames[k] + "' is not a SAM reference name"; return false; }
    if (!seen.insert(rnames[k]).second) { *err = "two sequences share the RNAME '" + rnames[k] + "'"; return false; }
    *out += "@SQ\tSN:" + rnames[k] + "\tLN:" + std::to_string(lengths[k]) + "\n";
  }
  *out += "@PG\tID:simmr-hip\tPN:simmr-hip\n";
  return true;
}

// A heap of the runs' next lines, smallest (key, run) on top; a run's lines are read through a window of its text so that
// the source is asked for large pieces, whatever the number of runs.
bool sam_merge_sorted_runs(const std::vector<SamSortedRun>& runs, const std::function<bool(uint64_t, size_t, char*)>& read,
                           const std::function<bool(const char*, size_t)>& write) {
  struct Cursor {
    size_t next = 0;          // the run's next line
    uint64_t at = 0;          // its place in the source
    std::vector<char> win;    // bytes [win_at, win_at + win.size()) of the source
    uint64_t win_at = 0;
  };
  constexpr size_t WINDOW = 1u << 20;
  std::vector<Cursor> cur(runs.size());
  typedef std::pair<uint64_t, size_t> Top;  // key, run number
  std::priority_queue<Top, std::vector<Top>, std::greater<Top>> heap;
  for (size_t k = 0; k < runs.size(); k++) {
    if (runs[k].key.size() != runs[k].len.size()) return false;
    cur[k].at = runs[k].offset;
    if (!runs[k].key.empty()) heap.emplace(runs[k].key[0], k);
  }
  std::string out;
  while (!heap.empty()) {
    const size_t k = heap.top().second;
    heap.pop();
    const SamSortedRun& run = runs[k];
    Cursor& c = cur[k];
    const size_t n = (size_t)run.len[c.next];
    if (c.at < c.win_at || c.at + n > c.win_at + c.win.size()) {  // the line is not in the window: refill from the line on
      uint64_t ahead = 0;  // whole lines, up to the window's size (one line at least)
      for (size_t i = c.next; i < run.len.size() && (i == c.next || ahead + run.len[i] <= WINDOW); i++) ahead += run.len[i];
      c.win.resize((size_t)ahead);
      c.win_at = c.at;
      if (ahead && !read(c.at, (size_t)ahead, c.win.data())) return false;
    }
    out.append(c.win.data() + (c.at - c.win_at), n);
    if (out.size() >= WINDOW) {
      if (!write(out.data(), out.size())) return false;
      out.clear();
    }
    c.at += n;
    if (++c.next < run.key.size()) heap.emplace(run.key[c.next], k);
  }
  return out.empty() || write(out.data(), out.size());
}

// --------------------------------------------------------------- ground truth per read
static const char* const TRUTH_TSV_HEADER = "read_id\tpair\tgenome_id\tsequence_id\tstart\tend\tstrand\tlength\tNM\tedits\n";

// the line of read r; gid / sid: its genome's and sequence's id
static void truth_line(std::string* out, uint64_t r, bool paired, uint32_t read_id, const char* gid, const char* sid, uint64_t start,
                       uint64_t end, uint8_t flags, uint32_t nm, const uint64_t* edit_off, const uint32_t* edit_pos,
                       const uint8_t* edit_ref, const uint8_t* edit_alt, const uint8_t* edit_qual, uint32_t qual_offset) {
  char buf[160];
  const uint64_t len = end > start ? end - start : start - end;
  snprintf(buf, sizeof buf, "%u\t%d\t", read_id, paired ? (int)(r & 1) + 1 : 0);
  *out += buf; *out += gid; *out += '\t'; *out += sid;
  snprintf(buf, sizeof buf, "\t%llu\t%llu\t%c\t%llu\t%u\t", (unsigned long long)start, (unsigned long long)end,
           (flags & SIMMR_FLAG_REVCOMP) ? '-' : '+', (unsigned long long)len, nm);
  *out += buf;
  if (edit_off[r] == edit_off[r + 1]) *out += '*';
  for (uint64_t i = edit_off[r]; i < edit_off[r + 1]; i++) {
    snprintf(buf, sizeof buf, "%s%u:%c>%c:%d", i > edit_off[r] ? "," : "", edit_pos[i], (char)edit_ref[i], (char)edit_alt[i],
             (int)edit_qual[i] - (int)qual_offset);
    *out += buf;
  }
  *out += '\n';
}

bool write_truth_tsv(const std::vector<Genome>& genomes, const HostReads& reads, const HostTruth& t, uint32_t qual_offset,
                     const std::string& output, bool with_header, std::string* err) {
  OutFile out(output, true);
  if (with_header) out.append(TRUTH_TSV_HEADER);
  std::string line;
  for (uint64_t r = 0; r < reads.n_reads && out.ok(); r++) {
    if (reads.genome[r] >= genomes.size() || reads.contig[r] >= genomes[reads.genome[r]].sequence.size()) {
      *err = "read " + std::to_string(r) + " names a genome or sequence the run does not have";
      return false;
    }
    const Genome& g = genomes[reads.genome[r]];
    line.clear();
    truth_line(&line, r, reads.paired, reads.read_id[r], g.uuid.c_str(), g.sequence[reads.contig[r]].id.c_str(), reads.start[r],
               reads.end[r], reads.flags[r], t.nm[r], t.edit_off.data(), t.edit_pos.data(), t.edit_ref.data(), t.edit_alt.data(),
               t.edit_qual.data(), qual_offset);
    out.append(line);
  }
  return out.close(err);
}

// --------------------------------------------------------------- strain sites
bool write_strain_sites_tsv(const Genome& genome, const HostStrainSites& s, const std::string& output, bool with_header,
                            std::string* err) {
  OutFile out(output, true);
  if (with_header) out.append("genome_id\tsequence_id\tposition\tref\talt\n");
  char buf[64];
  std::string line;
  for (size_t i = 0; i < s.pos.size() && out.ok(); i++) {
    if (s.contig[i] >= genome.sequence.size()) { *err = "site " + std::to_string(i) + " names a sequence the genome does not have"; return false; }
    line = genome.uuid; line += '\t'; line += genome.sequence[s.contig[i]].id;
    snprintf(buf, sizeof buf, "\t%llu\t%c\t%c\n", (unsigned long long)s.pos[i], (char)s.ref[i], (char)s.alt[i]);
    line += buf;
    out.append(line);
  }
  return out.close(err);
}

// the class of the statistics and pileup passes: A C G T are 0 1 2 3, every other byte 4
static int base_class(uint8_t b) { return b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : 4; }

bool write_strain_vcf(const std::vector<Genome>& genomes, const std::vector<std::vector<uint64_t>>& contig_len, const HostStrainSites& s,
                      const std::vector<uint32_t>& site_genome, const std::vector<uint32_t>& counts, const std::string& output,
                      std::string* err) {
  const size_t n = s.pos.size();
  if (site_genome.size() != n || s.contig.size() != n || s.ref.size() != n || s.alt.size() != n || counts.size() != n * 10) { *err = "the site columns and the count table differ in length"; return false; }
  OutFile out(output, false);
  out.append("##fileformat=VCFv4.2\n##source=simmr-hip\n");
  for (size_t g = 0; g < genomes.size(); g++)
    for (size_t c = 0; c < genomes[g].sequence.size(); c++) {
      if (g >= contig_len.size() || c >= contig_len[g].size()) { *err = "no length for sequence " + std::to_string(c) + " of genome " + std::to_string(g); return false; }
      out.append("##contig=<ID=" + genomes[g].uuid + "|" + genomes[g].sequence[c].id + ",length=" + std::to_string(contig_len[g][c]) + ">\n");
    }
  out.append("##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Reads of the run that cover the site (mates count separately)\">\n"
             "##INFO=<ID=AD,Number=R,Type=Integer,Description=\"Reads that show the reference and the alternate base\">\n"
             "##INFO=<ID=ADF,Number=R,Type=Integer,Description=\"The same among forward reads\">\n"
             "##INFO=<ID=ADR,Number=R,Type=Integer,Description=\"The same among reverse reads\">\n"
             "##INFO=<ID=OTH,Number=1,Type=Integer,Description=\"Reads that show neither: a third base or N\">\n"
             "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n");
  char buf[256];
  std::string line;
  for (size_t i = 0; i < n && out.ok(); i++) {
    if (site_genome[i] >= genomes.size() || s.contig[i] >= genomes[site_genome[i]].sequence.size()) { *err = "site " + std::to_string(i) + " names a sequence the run does not have"; return false; }
    const Genome& g = genomes[site_genome[i]];
    const uint32_t* k = counts.data() + i * 10;  // [strand][class]
    const int r = base_class(s.ref[i]), a = base_class(s.alt[i]);
    uint64_t dp = 0;
    for (int j = 0; j < 10; j++) dp += k[j];
    const uint64_t ad_r = (uint64_t)k[r] + k[5 + r], ad_a = (uint64_t)k[a] + k[5 + a];
    line = g.uuid; line += '|'; line += g.sequence[s.contig[i]].id;
    snprintf(buf, sizeof buf, "\t%llu\t.\t%c\t%c\t.\t.\tDP=%llu;AD=%llu,%llu;ADF=%u,%u;ADR=%u,%u;OTH=%llu\n", (unsigned long long)s.pos[i] + 1,
             (char)s.ref[i], (char)s.alt[i], (unsigned long long)dp, (unsigned long long)ad_r, (unsigned long long)ad_a, k[r], k[a], k[5 + r], k[5 + a],
             (unsigned long long)(dp - ad_r - ad_a));
    line += buf;
    out.append(line);
  }
  return out.close(err);
}

// --------------------------------------------------------------- run statistics
std::string fit_model_bytes(const simmr_fit_info& f, const simmr_fit_out& c) {
  simmr::ModelHost m;
  m.bin_size = 1;
  m.quality.resize(f.n_positions);
  for (uint64_t p = 0; p < f.n_positions; p++) {
    simmr::BinsHost& b = m.quality[p];
    b.num_bins = 70;
    b.bin_width = 1;
    b.density.assign(c.qual_density + p * SIMMR_FIT_DENSITIES, c.qual_density + (p + 1) * SIMMR_FIT_DENSITIES);
    for (uint32_t i = 0; i < 70; i++) b.ranges.emplace_back(i, i);
  }
  m.bit_encoding = 3;
  m.kmer_size = f.k;
  m.probabilities.resize(f.n_ref_kmers);
  for (uint64_t i = 0; i < f.n_ref_kmers; i++) {
    m.probabilities[i].first = c.kmer_ref[i];
    for (uint64_t j = c.kmer_first[i]; j < c.kmer_first[i + 1] && j < f.n_pairs; j++) m.probabilities[i].second.emplace_back(c.pair_alt[j], c.pair_prob[j]);
  }
  auto bins = [](uint64_t n, uint64_t width, const double* d, const uint32_t* lo, const uint32_t* hi) {
    simmr::BinsHost b;
    b.num_bins = n;
    b.bin_width = width;
    b.density.assign(d, d + n);
    for (uint64_t i = 0; i < n; i++) b.ranges.emplace_back(lo[i], hi[i]);
    return b;
  };
  m.insert_size_mean = f.insert_size_mean;
  m.insert_size_std = f.insert_size_std;
  m.has_insert_bins = f.n_insert_bins > 0;
  if (m.has_insert_bins) m.insert_bins = bins(f.n_insert_bins, f.insert_bin_width, c.insert_density, c.insert_lo, c.insert_hi);
  m.read_length_mean = f.read_length_mean;
  m.read_length_std = f.read_length_std;
  m.read_length_bins = bins(f.n_length_bins, f.length_bin_width, c.length_density, c.length_lo, c.length_hi);
  m.is_long = f.is_long != 0;
  return simmr::serialize_model(m);
}
bool write_fit_model(const simmr_fit_info& info, const simmr_fit_out& cols, const std::string& output, std::string* err) {
  OutFile f(output, false);
  f.append(fit_model_bytes(info, cols));
  return f.close(err);
}

bool write_stats_tsv(const simmr_run_stats& st, const std::string& output, std::string* err) {
  std::string text = "table\tset\ti\tj\tcount\n";
  char buf[96];
  auto row = [&](const char* table, int set, int i, int j, uint64_t count) {
    if (!count) return;
    auto idx = [&](int v) { if (v < 0) text += "\t-"; else { snprintf(buf, sizeof buf, "\t%d", v); text += buf; } };
    text += table; idx(set); idx(i); idx(j);
    snprintf(buf, sizeof buf, "\t%llu\n", (unsigned long long)count);
    text += buf;
  };
  for (int m = 0; m < 2; m++) row("reads", m, -1, -1, st.reads[m]);
  for (int m = 0; m < 2; m++) row("bases", m, -1, -1, st.bases[m]);
  for (int q = 0; q < 256; q++) row("qual_n", -1, q, -1, st.qual_n[q]);
  for (int q = 0; q < 256; q++) row("qual_mismatch", -1, q, -1, st.qual_mismatch[q]);
  for (int a = 0; a < 5; a++) for (int b = 0; b < 5; b++) row("pair", -1, a, b, st.pair[a][b]);
  for (int i = 0; i < (int)SIMMR_STATS_NM_BINS; i++) row("nm_hist", -1, i, -1, st.nm_hist[i]);
  for (int i = 0; i < 101; i++) row("gc_hist", -1, i, -1, st.gc_hist[i]);
  for (int m = 0; m < 2; m++) for (int j = 0; j < (int)SIMMR_STATS_CYCLES; j++) row("cycle_n", m, j, -1, st.cycle_n[m][j]);
  for (int m = 0; m < 2; m++) for (int j = 0; j < (int)SIMMR_STATS_CYCLES; j++) row("cycle_qsum", m, j, -1, st.cycle_qsum[m][j]);
  for (int m = 0; m < 2; m++) for (int j = 0; j < (int)SIMMR_STATS_CYCLES; j++) row("cycle_mismatch", m, j, -1, st.cycle_mismatch[m][j]);
  for (int m = 0; m < 2; m++) for (int j = 0; j < (int)SIMMR_STATS_CYCLES; j++) for (int c = 0; c < 5; c++) row("cycle_base", m, j, c, st.cycle_base[m][j][c]);
  OutFile out(output, false);
  out.append(text);
  return out.close(err);
}

// --------------------------------------------------------------- coverage depth
// genome id and sequence id of a row, or nullptr with *err set
static const Seq* depth_row_names(const std::vector<Genome>& genomes, const simmr_depth_contig& r, std::string* err) {
  if (r.genome >= genomes.size() || r.contig >= genomes[r.genome].sequence.size()) {
    *err = "a depth row names a genome or sequence the run does not have";
    return nullptr;
  }
  return &genomes[r.genome].sequence[r.contig];
}

bool write_depth_tsv(const std::vector<Genome>& genomes, const simmr_depth_contig* rows, uint64_t n_rows, const std::string& output,
                     std::string* err) {
  std::string text = "genome_id\tsequence_id\tlength\tcovered\tdepth_sum\tdepth_max\n";
  char buf[128];
  for (uint64_t k = 0; k < n_rows; k++) {
    const Seq* s = depth_row_names(genomes, rows[k], err);
    if (!s) return false;
    text += genomes[rows[k].genome].uuid; text += '\t'; text += s->id;
    snprintf(buf, sizeof buf, "\t%llu\t%llu\t%llu\t%u\n", (unsigned long long)rows[k].len, (unsigned long long)rows[k].covered,
             (unsigned long long)rows[k].depth_sum, rows[k].depth_max);
    text += buf;
  }
  OutFile out(output, false);  // (opened once every row is known to be good: a refused row leaves the old file)
  out.append(text);
  return out.close(err);
}

bool write_depth_track_tsv(const std::vector<Genome>& genomes, const simmr_depth_contig* rows, uint64_t n_rows, uint32_t window,
                           const uint64_t* win_sum, const uint32_t* win_covered, const uint32_t* win_max, const std::string& output,
                           std::string* err) {
  if (window == 0) { *err = "a depth track needs a window of at least one position"; return false; }
  OutFile out(output, false);
  out.append("genome_id\tsequence_id\tstart\tend\tdepth_sum\tcovered\tdepth_max\n");
  char buf[160];
  for (uint64_t k = 0; k < n_rows; k++) {
    const Seq* s = depth_row_names(genomes, rows[k], err);
    if (!s) return false;
    const std::string head = genomes[rows[k].genome].uuid + "\t" + s->id;
    uint64_t w = rows[k].first_window;
    for (uint64_t x = 0; x < rows[k].len && out.ok(); x += window, w++) {
      out.append(head);
      snprintf(buf, sizeof buf, "\t%llu\t%llu\t%llu\t%u\t%u\n", (unsigned long long)x, (unsigned long long)std::min<uint64_t>(x + window, rows[k].len),
               (unsigned long long)win_sum[w], win_covered[w], win_max[w]);
      out.append(buf, strlen(buf));
    }
  }
  return out.close(err);
}

// --------------------------------------------------------------- gold-standard assembly
// the sequence a region lies on, or nullptr with *err set; the columns must agree in length and seq_off must ascend inside seq
static const Seq* region_names(const std::vector<Genome>& genomes, const HostRegions& r, size_t k, bool with_seq, std::string* err) {
  if (r.genome[k] >= genomes.size() || r.contig[k] >= genomes[r.genome[k]].sequence.size()) {
    *err = "region " + std::to_string(k) + " names a genome or sequence the run does not have";
    return nullptr;
  }
  if (with_seq && (r.seq_off[k] > r.seq.size() || r.len[k] > r.seq.size() - r.seq_off[k])) {
    *err = "region " + std::to_string(k) + " leaves the base stream";
    return nullptr;
  }
  return &genomes[r.genome[k]].sequence[r.contig[k]];
}
static bool region_columns_agree(const HostRegions& r, std::string* err) {
  const size_t n = r.genome.size();
  if (r.contig.size() == n && r.start.size() == n && r.len.size() == n && r.depth_sum.size() == n && r.seq_off.size() == n + 1) return true;
  *err = "the region columns differ in length";
  return false;
}

bool write_gold_fasta(const std::vector<Genome>& genomes, const HostRegions& r, const std::string& output, std::string* err) {
  if (!region_columns_agree(r, err)) return false;
  for (size_t k = 0; k < r.genome.size(); k++)
    if (!region_names(genomes, r, k, true, err)) return false;
  OutFile out(output, false);  // (opened once every region is known to be good: a refused one leaves the old file)
  char buf[96];
  for (size_t k = 0; k < r.genome.size() && out.ok(); k++) {
    const Seq* s = region_names(genomes, r, k, true, err);
    out.append(">" + genomes[r.genome[k]].uuid + "|" + s->id);
    snprintf(buf, sizeof buf, ":%llu-%llu depth_sum=%llu\n", (unsigned long long)(r.start[k] + 1), (unsigned long long)(r.start[k] + r.len[k]),
             (unsigned long long)r.depth_sum[k]);
    out.append(buf, strlen(buf));
    const uint8_t* b = r.seq.data() + r.seq_off[k];
    for (uint64_t at = 0; at < r.len[k]; at += 80) {
      out.append(b + at, (size_t)std::min<uint64_t>(80, r.len[k] - at));
      out.append("\n", 1);
    }
  }
  return out.close(err);
}

bool write_gold_regions_tsv(const std::vector<Genome>& genomes, const HostRegions& r, const std::string& output, std::string* err) {
  if (!region_columns_agree(r, err)) return false;
  for (size_t k = 0; k < r.genome.size(); k++)
    if (!region_names(genomes, r, k, false, err)) return false;
  OutFile out(output, false);
  out.append("genome_id\tsequence_id\tstart\tlength\tdepth_sum\tseq_off\n");
  char buf[128];
  for (size_t k = 0; k < r.genome.size() && out.ok(); k++) {
    out.append(genomes[r.genome[k]].uuid + "\t" + genomes[r.genome[k]].sequence[r.contig[k]].id);
    snprintf(buf, sizeof buf, "\t%llu\t%llu\t%llu\t%llu\n", (unsigned long long)r.start[k], (unsigned long long)r.len[k],
             (unsigned long long)r.depth_sum[k], (unsigned long long)r.seq_off[k]);
    out.append(buf, strlen(buf));
  }
  return out.close(err);
}

// --------------------------------------------------------------- error profiles

static simmr_error_profile zero_pod() {
  simmr_error_profile p;
  memset(&p, 0, sizeof p);
  return p;
}
simmr_error_profile PerfectShortErrorProfile::pod() const {
  simmr_error_profile p = zero_pod();
  p.kind = SIMMR_PERFECT_SHORT; p.read_length = read_length; p.insert_size = insert_size;
  return p;
}
simmr_error_profile MinimalShortErrorProfile::pod() const {
  simmr_error_profile p = zero_pod();
  p.kind = SIMMR_MINIMAL_SHORT; p.read_length = read_length; p.insert_size = insert_size;
  p.mean_phred = mean_phred_score; p.read_length_std = read_length_std; p.insert_size_std = insert_size_std;
  return p;
}
simmr_error_profile MinimalLongErrorProfile::pod() const {
  simmr_error_profile p = zero_pod();
  p.kind = SIMMR_MINIMAL_LONG; p.mean_phred = mean_phred_score; p.length_mode = length_mode;
  p.long_start_mode = long_start_mode;
  // minimal_long.rs:64-69: shape = (mean / std_dev).powf(2.0); scale = std_dev.powf(2.0) / mean (f32)
  p.gamma_shape = powf(gamma_mean / gamma_std, 2.0f);
  p.gamma_scale = powf(gamma_std, 2.0f) / gamma_mean;
  return p;
}
simmr_error_profile PerfectLongErrorProfile::pod() const {
  simmr_error_profile p = MinimalLongErrorProfile::pod();
  p.kind = SIMMR_PERFECT_LONG;
  return p;
}

std::unique_ptr<CustomShortErrorProfile> CustomShortErrorProfile::from_path(const std::string& path, std::string* err) {
  std::ifstream f(path, std::ios::binary);
  if (!f) { *err = "No such file or directory (os error 2)"; return nullptr; }
  auto p = std::make_unique<CustomShortErrorProfile>();
  p->model.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
  simmr::ModelHost m;
  if (!simmr::parse_model(p->model.data(), p->model.size(), &m, err)) return nullptr;
  p->read_length_mean = m.read_length_mean;
  p->insert_size_mean = m.insert_size_mean;
  p->is_long = m.is_long;
  return p;
}
simmr_error_profile CustomShortErrorProfile::pod() const {
  simmr_error_profile p = zero_pod();
  p.kind = SIMMR_CUSTOM;
  p.custom_model = model.data();
  p.custom_model_bytes = model.size();
  p.length_mode = length_mode;          // (set for long-read models only: determine_error_profile)
  p.long_start_mode = long_start_mode;
  return p;
}
uint16_t CustomShortErrorProfile::minimum_genome_size() const {
  const double v = 2.0 * read_length_mean + insert_size_mean;  // `as u16` saturates
  if (!(v == v) || v <= 0.0) return 0;
  return v >= 65535.0 ? 65535 : (uint16_t)v;
}

// ----------------------------------------------------------- abundance profiles

Abundances AbundanceProfile::adjust_for_size(const std::vector<Genome>& genomes, const Abundances& ra,
                                             uint64_t, bool) const {
  // uniform.rs:79-94 == custom.rs:80-95 (total_coverage is computed there but unused)
  double total_reads = 0.0, total_adjusts = 0.0;
  for (const auto& x : ra) total_reads += (double)x.first;
  for (size_t i = 0; i < genomes.size() && i < ra.size(); i++) total_adjusts += (double)genomes[i].size * ra[i].second;
  Abundances out;
  for (size_t i = 0; i < genomes.size() && i < ra.size(); i++)
    out.emplace_back((uint64_t)ceil(total_reads * ((ra[i].second * (double)genomes[i].size) / total_adjusts)), ra[i].second);
  return out;
}
Abundances UniformAbundanceProfile::determine_abundances(uint64_t total_reads, uint64_t num_genomes) const {
  const uint64_t per = (uint64_t)ceil((double)total_reads / (double)num_genomes);  // uniform.rs:28
  return Abundances(num_genomes, {per, 100.0 / (double)num_genomes});
}
Abundances ExactAbundanceProfile::determine_abundances(uint64_t total_reads, uint64_t num_genomes) const {
  return Abundances(num_genomes, {total_reads, 100.0 / (double)num_genomes});        // exact.rs:17-24
}
Abundances CustomAbundanceProfile::determine_abundances(uint64_t total_reads, uint64_t) const {
  double total = 0.0;                                                                // custom.rs:26-48
  for (double a : abundances) total += a;
  Abundances out;
  if (total < 0.99 || total > 1.01)
    for (double a : abundances) out.emplace_back((uint64_t)ceil((double)total_reads * (a / total)), a / total);
  else
    for (double a : abundances) out.emplace_back((uint64_t)ceil((double)total_reads * a), a);
  return out;
}

// ------------------------------------------------------------------------ cli.rs

std::string usage() {
  return "simmr-hip — simmr's read simulation on MI355X (same flags as simmr, cli.rs:93-220)\n"
         "  --genome <FILE>...            Filepath to a genome to use for simulations\n"
         "  --genome-file <FILE>          TSV of genome filepaths and metadata (path, uuid|id, abundance)\n"
         "  --output <FILE>               FASTQ output containing simulated reads (required)\n"
         "  --num-reads <N>               Number of reads to simulate [default: 1000]\n"
         "  --read-length <N>             Individual read length (nt) [default: 150]\n"
         "  --read-length-std <F>         Standard deviation of read lengths [default: 10]\n"
         "  --insert-size <N>             Insert size for PE reads (nt) [default: 150]\n"
         "  --mean-phred-score <N>        Average Phred quality score [default: 30]\n"
         "  --error-profile <P>           minimal-short | minimal-long | perfect-short | perfect-long | custom-short [default: perfect-short]\n"
         "                                (extension: custom-long = a simmrd long-read model through the long-read path,\n"
         "                                 which the reference's own enum cannot select, cli.rs:62-70)\n"
         "  --abundance-profile <P>       exact | uniform | custom [default: uniform]\n"
         "  --custom-profile <FILE>       Filepath to a custom error profile (simmrd model) for custom-short\n"
         "  --with-ani <N>                Generate reads with an average identity of N percent (25 .. 100, decimals accepted)\n"
         "                                compared to their reference: every genome becomes a strain, with the same substitutions\n"
         "                                in every read that covers a site (declared and never read in the reference, cli.rs:185-191)\n"
         "  --read-header-format <FMT>    header template ({:genome_id:} {:read_id:} {:pair:} {:sequence_id:} ...)\n"
         "  --seed <N>                    Random seed\n"
         "  --size-adjusted               Adjust by genome size\n"
         "  --contiguous                  Treat separate sequences in a genome as one contiguous sequence\n"
         "extensions: --device <N>  --devices <a,b,...>  --gamma <mean,std>  --per-read-lengths  --uniform-start  --host-fastq  --host-normalize  --device-chunk-reads <N>  --rng <reference|philox|philox-full>\n"
         "            --truth <FILE>  per-read ground truth as a TSV: read_id pair genome_id sequence_id start end strand length NM edits\n"
         "                            (edits: * or pos:REF>ALT:Q, ...; found on the device by comparing every read with the staged genome;\n"
         "                             not with --devices)\n"
         "            --sam <FILE>    the true alignments as SAM: @HD / @SQ / @PG, then one line per read in read order with FLAG, the mate\n"
         "                            fields, SEQ and QUAL on the forward strand, NM:i: and MD:Z: (CIGAR <L>M, MAPQ 255, unsorted, no @RG);\n"
         "                            formatted on the device from the reads and their ground truth (turns the truth pass on); RNAME is the\n"
         "                            first word of the sequence id and must be unique in the run; QNAME is the read id, so\n"
         "                            --read-header-format '@{:read_id:}/{:pair:}' makes the FASTQ names match; combines with --truth;\n"
         "                            not with --devices\n"
         "            --sam-sorted    the file of --sam in coordinate order, under @HD SO:coordinate: the lines ascend by (@SQ index, POS),\n"
         "                            ties in read order, across every range of the run (each range is sorted on the device; several\n"
         "                            ranges are merged through a temporary file beside FILE); needs --sam; not with --devices\n"
         "            --bam <FILE>    the same alignments as BAM, in read order: the header of --sam (unsorted) and one record per read, written\n"
         "                            and framed into BGZF blocks on the device; the blocks are stored, not compressed (what samtools view -u\n"
         "                            writes: samtools sort, samtools index after it, and bgzip recompress them); no index, no @RG; the\n"
         "                            RNAME rules of --sam; combines with --sam and --truth; not with --devices\n"
         "            --bam-sorted    the file of --bam in coordinate order, under @HD SO:coordinate, and its BAI index written beside it as\n"
         "                            FILE.bai (--bam-index <FILE> names another place): sorted and indexed on the device, across every\n"
         "                            range of the run (several ranges are merged through a temporary file beside FILE); a genome browser\n"
         "                            or a region query opens the pair directly; the blocks are stored, not compressed; every sequence\n"
         "                            stays below 2^29 bases (the reach of a BAI index; no CSI); needs --bam; not with --devices\n"
         "            --overlaps <FILE>  the true read-to-read overlaps of the run as PAF: one record per pair of reads that share at least\n"
         "                            --min-overlap reference bases of one sequence, across every range of the run, found and formatted on\n"
         "                            the device; names as --sam's QNAME (the read id, /1 or /2 for pairs); columns 10 and 11 carry the\n"
         "                            length of the shared reference interval; not with --devices\n"
         "            --min-overlap <N>  shared reference bases from which two reads overlap [default: 1]\n"
         "            --eval-overlaps <FILE>  no simulation: score an overlapper's PAF (plain text, as minimap2 -x ava-ont writes it) against the\n"
         "                            true overlaps of --eval-overlaps-truth, joined by the two read names and classified on the device: a record\n"
         "                            is correct when it names a true pair on the true relative strand and, on both reads, its interval and\n"
         "                            the true one overlap by at least --eval-overlaps-min-pct percent of their union; takes only\n"
         "                            --eval-overlaps-truth, --eval-overlaps-report, --eval-overlaps-pairs, --eval-overlaps-min-pct and --device\n"
         "                            (no genomes, no --output, not --devices)\n"
         "            --eval-overlaps-truth <FILE>  the file of --overlaps for the reads that were overlapped\n"
         "            --eval-overlaps-report <FILE>  the result as a TSV: the counts as #name value lines, #sensitivity (true pairs found) and\n"
         "                            #precision (records correct), then a row per bit length of the true overlap with pairs: L, bits, found,\n"
         "                            not found\n"
         "            --eval-overlaps-pairs <FILE>  every true pair: the two read names, the true overlap's length on the query, the class of its\n"
         "                            best record (0 no record, 2 wrong, 3 correct), records\n"
         "            --eval-overlaps-min-pct <PCT>  1 .. 100 [default: 10]\n"
         "            --eval-vcf <FILE>  no simulation: score a variant caller's VCF (plain text, as bcftools call -mv writes it) against the strain's\n"
         "                            sites of --eval-vcf-truth, joined by contig and position and classified on the device: a call is an\n"
         "                            ALT base that differs from REF (an MNP gives one per changed base; of the first sample's GT only the\n"
         "                            called alleles count), correct when the site exists with that reference and alternate base; indels and\n"
         "                            symbolic alleles are counted and not scored; takes only --eval-vcf-truth, --eval-vcf-report,\n"
         "                            --eval-vcf-sites, --eval-vcf-filtered and --device (no genomes, no --output, not --devices)\n"
         "            --eval-vcf-truth <FILE>  the file of --strain-vcf for the reads that were called; its ##contig lines name the contigs\n"
         "            --eval-vcf-report <FILE>  the result as a TSV: the counts as #name value lines, #precision (calls correct) and #recall\n"
         "                            (sites found) as fractions and percentages, a Q row per QUAL row with calls from 255 downward with\n"
         "                            the cumulative precision and correct calls per site, an AD row per bit length of the reads that\n"
         "                            showed the alternate base: found, not found\n"
         "            --eval-vcf-sites <FILE>  every true site: contig, position, ref, alt, reads that showed alt, the class of its best call\n"
         "                            (0 no call, 2 wrong, 3 correct), that call's QUAL row, calls\n"
         "            --eval-vcf-filtered  score the records whose FILTER is neither . nor PASS too\n"
         "            --eval-classified <FILE>  no simulation: score a read classifier's per-read output (plain text, the columns of Kraken 2: C or U,\n"
         "                            the read name, the taxid, also as 'name (taxid N)') against the genome of every read in the file of\n"
         "                            --eval-classified-truth, joined by read id and classified per rank on the device: correct, above\n"
         "                            (right but less specific), wrong, unclassified; takes only --eval-classified-truth, --eval-taxonomy,\n"
         "                            --eval-genome-taxa, --eval-classified-report, --eval-classified-reads, --eval-classified-taxa and\n"
         "                            --device (no genomes, no --output, not --devices)\n"
         "            --eval-classified-truth <FILE>  the file of --truth for the reads that were classified\n"
         "            --eval-taxonomy <FILE>  the tree: NCBI's nodes.dmp, or taxid, parent and rank as a TSV (merged.dmp is not read)\n"
         "            --eval-genome-taxa <FILE>  genome_id and taxid as a TSV, a line per genome of the truth\n"
         "            --eval-classified-report <FILE>  the result as a TSV: the counts as #name value lines, an R row per rank with the records and\n"
         "                            the reads by class, a P row per rank with precision, sensitivity and F1 on both, an A row per rank with\n"
         "                            the L1 distance between the true and the called abundance profile (by reads)\n"
         "            --eval-classified-reads <FILE>  every true read: id, genome, lines, records, the best class at each of the 8 ranks\n"
         "            --eval-classified-taxa <FILE>  every taxon with reads: taxid, rank, true, called, both (clade sums), precision, recall\n"
         "            --eval-assembly <FILE>  no simulation: score an assembler's contigs (plain FASTA) against the gold-standard assembly of\n"
         "                            --eval-assembly-truth by canonical k-mers, looked up on the device: completeness per genome, the\n"
         "                            k-mers in no genome and the consensus quality they give, the genome of every contig; takes only\n"
         "                            --eval-assembly-truth, --eval-assembly-report, --eval-assembly-contigs, --eval-assembly-k and --device\n"
         "                            (no genomes, no --output, not --devices)\n"
         "            --eval-assembly-truth <FILE>  the file of --gold-assembly; the genomes are the header prefixes in front of '|'\n"
         "            --eval-assembly-report <FILE>  the result as a TSV: the counts as #name value lines, #completeness, #qv, the contiguity\n"
         "                            of both sides (records, bases, longest, N50) and a G row per genome\n"
         "            --eval-assembly-contigs <FILE>  every contig: name, length, kmers, found, shared, top genome row, its votes, its name\n"
         "            --eval-assembly-k <K>  k-mer size, odd, 15 .. 31 [default: 31]\n"
         "            --eval-placement <FILE>  no simulation: place an assembler's contigs (plain FASTA) on the gold-standard assembly of\n"
         "                            --eval-placement-truth by unique k-mers, on the device: collinear blocks, the breakpoints between them by\n"
         "                            class, the misassembled contigs.  Takes only --eval-placement-truth, --eval-placement-report, --eval-placement-blocks,\n"
         "                            --eval-placement-contigs, --eval-placement-k, --eval-placement-band, --eval-placement-relocation,\n"
         "                            --eval-placement-min-anchors and --device\n"
         "            --eval-placement-truth <FILE>  the file of --gold-assembly; the genomes are the header prefixes in front of '|'\n"
         "            --eval-placement-report <FILE>  the result as a TSV: the counts as #name value lines, #misassemblies, #NA50, #NGA50 and a G\n"
         "                            row per genome with its own NGA50 and its anchored fraction\n"
         "            --eval-placement-blocks <FILE>  every block: contig, q_start, q_end, truth record, p_start, p_end, strand, hits, join class\n"
         "            --eval-placement-contigs <FILE>  every contig: name, length, hits, blocks, first block, block bases, worst join class\n"
         "            --eval-placement-k <K>  k-mer size, odd, 15 .. 31 [default: 31]\n"
         "            --eval-placement-band <N>  two neighbouring hits lie on one diagonal where their diagonals differ by at most N [default: 64]\n"
         "            --eval-placement-relocation <N>  a step of more than N bases on one record and strand is a relocation [default: 1000]\n"
         "            --eval-placement-min-anchors <N>  a run of fewer hits is dropped [default: 16]\n"
         "            --eval-bins <FILE>  no simulation: score a binner's assignment (contig, tab, bin a line; '#' and '@' lines skipped) against\n"
         "                            the contigs file of --eval-bins-truth, joined by name on the device: purity, completeness, F1, the\n"
         "                            adjusted Rand index, CAMI's bin classes; takes only --eval-bins-truth, --eval-bins-report,\n"
         "                            --eval-bins-bins, --eval-bins-contigs and --device\n"
         "            --eval-bins-truth <FILE>  the file of --eval-assembly-contigs; the genomes are its distinct field-8 values other than '.'\n"
         "            --eval-bins-report <FILE>  the result as a TSV: the counts as #name value lines, the fractions, a G row per genome, a B row per bin\n"
         "            --eval-bins-bins <FILE>  every (bin, genome) cell: bin, genome, contigs, bases\n"
         "            --eval-bins-contigs <FILE>  every truth contig: name, length, genome, bin or '.', records\n"
         "            --eval-corrected <FILE>  no simulation: score a read error corrector's FASTQ against the true reads of --eval-corrected-truth,\n"
         "                            base by base on the device: kept, damaged, fixed, left, miscorrected, trimmed; gain, sensitivity,\n"
         "                            specificity; takes only --eval-corrected-truth, --eval-corrected-report, --eval-corrected-reads,\n"
         "                            --eval-corrected-fasta and --device\n"
         "            --eval-corrected-truth <FILE>  the file of --sam for the same run: SEQ, QUAL, the strand and MD:Z give every read's true bases\n"
         "            --eval-corrected-report <FILE>  the result as a TSV: the counts as #name value lines, the three ratios, rows by quality and by position, the cube\n"
         "            --eval-corrected-reads <FILE>  every read that is not its true self: id, mate, length, errors before, errors left or '.', records\n"
         "            --eval-corrected-fasta  the corrected reads are two-line FASTA ('>'name, bases), not FASTQ\n"
         "            --stats <FILE>  the run's statistics as a long-form TSV (table set i j count, non-zero entries): reads and bases per mate,\n"
         "                            bases and edits by Phred, expected x written base, edits per read, GC per read, and per cycle the\n"
         "                            reads, quality sum, edits and base composition; counted on the device; combines with --truth;\n"
         "                            not with --devices\n"
         "            --fit-model <FILE>  an error model fitted from the run, as `simmrd generate` writes it and --custom-profile reads it:\n"
         "                            k-mer to alternate-k-mer probabilities, a quality density per read position, read-length and insert-size\n"
         "                            densities, counted on the device over every range of the run; a quality above 93 is refused;\n"
         "                            not with --devices\n"
         "            --fit-k <K>  k-mer size of --fit-model, 3 .. 10 [default: 7]\n"
         "            --fit-max-alt <N>  alternates kept per reference k-mer [default: 20]\n"
         "            --fit-from-sam <FILE>  no simulation: fit the model of --fit-model from the alignments of a SAM file (plain text with\n"
         "                            CIGAR and MD:Z; no BAM, no gzip), parsed, filtered and counted on the device; what was taken and\n"
         "                            skipped goes to stderr; takes only --fit-model, --fit-k, --fit-max-alt, --single-reads and --device\n"
         "                            (no genomes, no --output, not --devices)\n"
         "            --single-reads  with --fit-from-sam: the reads are unpaired (no insert sizes are taken)\n"
         "            --depth <FILE>  coverage the run put on every sequence, as a TSV: genome_id sequence_id length covered depth_sum depth_max\n"
         "                            (read depth, mates counted separately; counted on the device from every range of the run;\n"
         "                             combines with --truth and --stats; not with --devices)\n"
         "            --depth-track <FILE>  the same per window: genome_id sequence_id start end depth_sum covered depth_max\n"
         "            --depth-window <W>    positions per window of --depth-track [default: 1000]\n"
         "            --gold-assembly <FILE>  the gold-standard assembly as FASTA: every stretch of a sequence the run covered, one record\n"
         "                            >genome_id|sequence_id:first-last depth_sum=N per stretch (1-based, closed), bases in lines of 80; found and\n"
         "                            read out on the device from the run's depth (turns the depth pass on); with --with-ani the bases\n"
         "                            are the strain's; not with --devices\n"
         "            --gold-regions <FILE>   the same stretches as a TSV: genome_id sequence_id start length depth_sum seq_off (start 0-based)\n"
         "            --gold-min-depth <D>    a position belongs to a stretch from this read depth on [default: 1]\n"
         "            --gold-min-length <M>   shorter stretches are left out [default: 1]\n"
         "            --strain-sites <FILE>  the sites --with-ani changed, as a TSV: genome_id sequence_id position ref alt (position 0-based;\n"
         "                            drawn and listed on the device; with --truth, which reports the sequencing errors against the strain,\n"
         "                            the full truth against the original assembly; needs --with-ani; with --devices written from the first)\n"
         "            --strain-vcf <FILE>  the same sites as VCF 4.2 with what the reads of this run show at each: DP, AD, ADF, ADR (reference and\n"
         "                            alternate base, all / forward / reverse reads) and OTH (a third base or N), mates counted separately;\n"
         "                            counted on the device from every range of the run; CHROM is genome_id|sequence_id, POS 1-based;\n"
         "                            needs --with-ani; combines with --strain-sites; not with --devices\n"
         "            --eval-sam <FILE>  no simulation: score an aligner's SAM (plain text) against the true alignments of --eval-truth, joined by\n"
         "                            QNAME (the read id) and mate and classified on the device: a mapped record is correct when it lies on the\n"
         "                            truth's sequence and strand and the two reference intervals overlap by at least --eval-min-overlap percent\n"
         "                            of their union (paftools mapeval's rule); takes only --eval-truth, --eval-report, --eval-reads,\n"
         "                            --eval-min-overlap and --device (no genomes, no --output, not --devices)\n"
         "            --eval-truth <FILE>  the file of --sam for the reads that were aligned (either order); its @SQ lines name the sequences\n"
         "            --eval-report <FILE>  the result as a TSV: the counts as #name value lines, then from MAPQ 255 downwards a row per MAPQ\n"
         "                            with records: Q, MAPQ, mapped, wrong, cumulative wrong / cumulative mapped, cumulative mapped\n"
         "            --eval-reads <FILE>  every true read whose best record is not correct: id, mate bit, class (0 no record, 1 unmapped,\n"
         "                            2 wrong), MAPQ, records\n"
         "            --eval-min-overlap <PCT>  1 .. 100 [default: 10]\n";
}

void mapeval_sq_names(const char* text, size_t n, std::vector<std::string>* names) {
  for (size_t a = 0; a < n;) {
    const char* nl = (const char*)memchr(text + a, '\n', n - a);
    const size_t b = nl ? (size_t)(nl - text) : n;  // the line is text[a, b)
    if (b - a >= 4 && memcmp(text + a, "@SQ\t", 4) == 0) {
      for (size_t f = a + 4; f < b;) {  // its fields
        const char* tab = (const char*)memchr(text + f, '\t', b - f);
        const size_t g = tab ? (size_t)(tab - text) : b;
        if (g - f >= 3 && memcmp(text + f, "SN:", 3) == 0) { names->emplace_back(text + f + 3, g - f - 3); break; }
        f = g + 1;
      }
    }
    a = b + 1;
  }
}

std::string mapeval_report(const uint64_t* counts, const uint64_t* by_mapq) {
  static const char* const NAMES[MAPEVAL_N_COUNTS] = {"truth_lines", "truth_header", "truth_entries", "truth_skipped", "lines", "header", "records",
                                                      "secondary", "cigar_op", "unknown_read", "unknown_ref", "unmapped", "correct", "wrong", "missing",
                                                      "multiple", "reads_correct", "reads_wrong", "reads_unmapped"};
  std::string out;
  for (size_t i = 0; i < MAPEVAL_N_COUNTS; i++) out += std::string("#") + NAMES[i] + "\t" + std::to_string((unsigned long long)counts[i]) + "\n";
  uint64_t cum_mapped = 0, cum_wrong = 0;
  for (int q = 255; q >= 0; q--) {
    const uint64_t ok = by_mapq[2 * q], wrong = by_mapq[2 * q + 1];
    if (ok + wrong == 0) continue;
    cum_mapped += ok + wrong;
    cum_wrong += wrong;
    char ratio[64];
    snprintf(ratio, sizeof ratio, "%.6g", (double)cum_wrong / (double)cum_mapped);
    out += "Q\t" + std::to_string(q) + "\t" + std::to_string((unsigned long long)(ok + wrong)) + "\t" + std::to_string((unsigned long long)wrong) + "\t" +
           ratio + "\t" + std::to_string((unsigned long long)cum_mapped) + "\n";
  }
  return out;
}

std::string mapeval_read_rows(const uint64_t* key, const uint32_t* best, const uint32_t* hits, size_t n) {
  std::string out;
  for (size_t i = 0; i < n; i++) {
    if ((best[i] >> 8) == 3u) continue;
    out += std::to_string((unsigned long long)(key[i] >> 1)) + "\t" + std::to_string((unsigned)(key[i] & 1u)) + "\t" + std::to_string(best[i] >> 8) + "\t" +
           std::to_string(best[i] & 255u) + "\t" + std::to_string(hits[i]) + "\n";
  }
  return out;
}

std::string ovleval_report(const uint64_t* counts, const uint64_t* by_len) {
  static const char* const NAMES[OVLEVAL_N_COUNTS] = {"truth_lines", "truth_entries", "truth_reads", "lines", "records", "unknown_read", "self", "no_pair",
                                                      "wrong_strand", "wrong_interval", "correct", "wrong", "pairs_found", "pairs_wrong", "pairs_missed",
                                                      "pairs_multiple"};
  std::string out;
  for (size_t i = 0; i < OVLEVAL_N_COUNTS; i++) out += std::string("#") + NAMES[i] + "\t" + std::to_string((unsigned long long)counts[i]) + "\n";
  auto ratio = [](uint64_t num, uint64_t den) -> std::string {
    if (den == 0) return "0";
    char text[64];
    snprintf(text, sizeof text, "%.6f", (double)num / (double)den);
    return text;
  };
  const uint64_t entries = counts[1], correct = counts[10], wrong = counts[11], found = counts[12];
  out += "#sensitivity\t" + ratio(found, entries) + "\n";
  out += "#precision\t" + ratio(correct, correct + wrong) + "\n";
  for (size_t b = 0; b < OVLEVAL_LEN_ROWS; b++) {
    if (by_len[2 * b] == 0 && by_len[2 * b + 1] == 0) continue;
    out += "L\t" + std::to_string(b) + "\t" + std::to_string((unsigned long long)by_len[2 * b]) + "\t" + std::to_string((unsigned long long)by_len[2 * b + 1]) + "\n";
  }
  return out;
}

std::string ovleval_pair_rows(const uint64_t* key_a, const uint64_t* key_b, const uint64_t* ov, const uint32_t* best, const uint32_t* hits, size_t n) {
  auto name = [](uint64_t key) { return std::to_string((unsigned long long)(key >> 1)) + (key & 1u ? "/2" : ""); };
  std::string out;
  for (size_t i = 0; i < n; i++)
    out += name(key_a[i]) + "\t" + name(key_b[i]) + "\t" + std::to_string((unsigned long long)ov[i]) + "\t" + std::to_string(best[i]) + "\t" +
           std::to_string(hits[i]) + "\n";
  return out;
}

void vcfeval_contig_names(const char* text, size_t n, std::vector<std::string>* names) {
  static const char KEY[] = "##contig=<ID=";
  const size_t k = sizeof KEY - 1;
  for (size_t a = 0; a < n;) {
    size_t b = a;
    while (b < n && text[b] != '\n') b++;
    if (b - a > k && memcmp(text + a, KEY, k) == 0) {
      size_t e = a + k;
      while (e < b && text[e] != ',' && text[e] != '>') e++;
      if (e > a + k) names->emplace_back(text + a + k, e - (a + k));
    }
    a = b + 1;
  }
}

std::string vcfeval_report(const uint64_t* counts, const uint64_t* by_qual, const uint64_t* by_ad) {
  static const char* const NAMES[VCFEVAL_N_COUNTS] = {"truth_lines", "truth_header", "truth_entries", "lines", "header", "records", "filtered", "qual_missing",
                                                      "ref_call", "symbolic", "indel", "long_allele", "ref_call_allele", "calls", "unknown_contig", "no_site",
                                                      "ref_mismatch", "wrong_allele", "correct", "wrong", "sites_found", "sites_wrong", "sites_missed",
                                                      "sites_multiple"};
  auto n = [](uint64_t v) { return std::to_string((unsigned long long)v); };
  std::string out;
  for (size_t i = 0; i < VCFEVAL_N_COUNTS; i++) out += std::string("#") + NAMES[i] + "\t" + n(counts[i]) + "\n";
  auto frac = [&](uint64_t num, uint64_t den) -> std::string {
    char text[64] = "0";
    if (den != 0) snprintf(text, sizeof text, "%.4f", 100.0 * (double)num / (double)den);
    return n(num) + "/" + n(den) + "\t" + text;
  };
  const uint64_t entries = counts[2], calls = counts[13], correct = counts[18], found = counts[20];
  out += "#precision\t" + frac(correct, calls) + "\n";
  out += "#recall\t" + frac(found, entries) + "\n";
  uint64_t cum_correct = 0, cum_calls = 0;
  for (size_t q = 256; q-- > 0;) {
    if (by_qual[2 * q] == 0 && by_qual[2 * q + 1] == 0) continue;
    cum_correct += by_qual[2 * q];
    cum_calls += by_qual[2 * q] + by_qual[2 * q + 1];
    out += "Q\t" + std::to_string(q) + "\t" + n(by_qual[2 * q]) + "\t" + n(by_qual[2 * q + 1]) + "\t" + frac(cum_correct, cum_calls) + "\t" +
           frac(cum_correct, entries) + "\n";
  }
  for (size_t b = 0; b < VCFEVAL_AD_ROWS; b++) {
    if (by_ad[2 * b] == 0 && by_ad[2 * b + 1] == 0) continue;
    out += "AD\t" + std::to_string(b) + "\t" + n(by_ad[2 * b]) + "\t" + n(by_ad[2 * b + 1]) + "\n";
  }
  return out;
}

std::string vcfeval_site_rows(const std::vector<std::string>& names, const uint64_t* key, const uint32_t* alleles, const uint32_t* ad, const uint32_t* best,
                              const uint32_t* hits, size_t n) {
  std::string out;
  for (size_t i = 0; i < n; i++) {
    const uint64_t row = key[i] >> 40, pos = (key[i] & ((1ull << 40) - 1)) + 1;
    out += row < names.size() ? names[row] : std::string("?");
    out += "\t" + std::to_string((unsigned long long)pos) + "\t" + "ACGT"[(alleles[i] >> 2) & 3u] + "\t" + "ACGT"[alleles[i] & 3u] + "\t" + std::to_string(ad[i]) +
           "\t" + std::to_string(best[i] >> 8) + "\t" + std::to_string(best[i] & 255u) + "\t" + std::to_string(hits[i]) + "\n";
  }
  return out;
}

// ---- --eval-assembly ------------------------------------------------------------------------------------------------------------------
void asmeval_fasta_records(const char* text, size_t n, std::vector<std::string>* first_word, std::vector<uint64_t>* length) {
  bool any = false;
  for (size_t a = 0; a < n;) {
    size_t b = a;
    while (b < n && text[b] != '\n') b++;
    size_t e = b;
    if (b < n && e > a && text[e - 1] == '\r') e--;  // (only directly before a '\n')
    if (e > a && text[a] == '>') {
      size_t w = a + 1;
      while (w < e && text[w] != ' ' && text[w] != '\t' && text[w] != '\r') w++;
      first_word->emplace_back(text + a + 1, w - (a + 1));
      length->push_back(0);
      any = true;
    } else if (any) {
      length->back() += e - a;
    }
    a = b + 1;
  }
}

void asmeval_contiguity(const uint64_t* length, size_t n, uint64_t out[4]) {
  std::vector<uint64_t> ls(length, length + n);
  std::sort(ls.begin(), ls.end(), std::greater<uint64_t>());
  uint64_t total = 0, run = 0;
  for (uint64_t x : ls) total += x;
  out[0] = n; out[1] = total; out[2] = n ? ls[0] : 0; out[3] = 0;
  for (uint64_t x : ls) {
    run += x;
    if (2 * run >= total) { out[3] = x; break; }
  }
}

std::string asmeval_report(const uint64_t* counts, uint32_t k, const std::vector<std::string>& genomes, const uint64_t* by_genome, const uint64_t* truth_length,
                           size_t n_truth, const uint64_t* contig_length, size_t n_contigs) {
  static const char* const NAMES[ASMEVAL_N_COUNTS] = {"truth_records", "truth_bases", "truth_invalid", "truth_kmers", "truth_distinct", "truth_shared_distinct",
                                                      "records", "bases", "invalid", "kmers", "found", "shared", "novel", "contigs_short", "contigs_novel",
                                                      "contigs_pure", "contigs_mixed", "contigs_shared_only"};
  auto n = [](uint64_t v) { return std::to_string((unsigned long long)v); };
  auto frac = [&](uint64_t num, uint64_t den) -> std::string {
    char text[64] = "NA";
    if (den != 0) snprintf(text, sizeof text, "%.6f", (double)num / (double)den);
    return text;
  };
  std::string out;
  for (size_t i = 0; i < ASMEVAL_N_COUNTS; i++) out += std::string("#") + NAMES[i] + "\t" + n(counts[i]) + "\n";
  out += "#k\t" + std::to_string(k) + "\n";
  uint64_t distinct = 0, distinct_found = 0;
  for (size_t g = 0; g <= genomes.size(); g++) {
    distinct += by_genome[g * ASMEVAL_GENOME_COLS];
    distinct_found += by_genome[g * ASMEVAL_GENOME_COLS + 1];
  }
  out += "#completeness\t" + n(distinct_found) + "/" + n(distinct) + "\t" + frac(distinct_found, distinct) + "\n";
  const uint64_t kmers = counts[9], novel = counts[12];
  char qv[64] = "NA";
  if (kmers != 0 && novel == 0) snprintf(qv, sizeof qv, "inf");
  else if (kmers != 0) snprintf(qv, sizeof qv, "%.4f", -10.0 * log10(1.0 - pow(1.0 - (double)novel / (double)kmers, 1.0 / (double)k)));
  out += std::string("#qv\t") + qv + "\n";
  uint64_t c[4];
  asmeval_contiguity(truth_length, n_truth, c);
  out += "#truth_contiguity\t" + n(c[0]) + "\t" + n(c[1]) + "\t" + n(c[2]) + "\t" + n(c[3]) + "\n";
  asmeval_contiguity(contig_length, n_contigs, c);
  out += "#contigs_contiguity\t" + n(c[0]) + "\t" + n(c[1]) + "\t" + n(c[2]) + "\t" + n(c[3]) + "\n";
  out += "#G\tgenome\tdistinct\tdistinct_found\tover\tcontigs\tcontig_bases\tcompleteness\n";
  for (size_t g = 0; g <= genomes.size(); g++) {
    const uint64_t* r = by_genome + g * ASMEVAL_GENOME_COLS;
    out += "G\t" + (g < genomes.size() ? genomes[g] : std::string("shared"));
    for (size_t j = 0; j < ASMEVAL_GENOME_COLS; j++) out += "\t" + n(r[j]);
    out += "\t" + frac(r[1], r[0]) + "\n";
  }
  return out;
}

std::string asmeval_contig_rows(const std::vector<std::string>& names, const std::vector<std::string>& genomes, const uint64_t* length, const uint32_t* kmers,
                                const uint32_t* found, const uint32_t* shared, const uint32_t* top_genome, const uint32_t* top_kmers, size_t n) {
  std::string out;
  for (size_t i = 0; i < n; i++) {
    out += i < names.size() ? names[i] : std::string("?");
    out += "\t" + std::to_string((unsigned long long)length[i]) + "\t" + std::to_string(kmers[i]) + "\t" + std::to_string(found[i]) + "\t" +
           std::to_string(shared[i]) + "\t" + std::to_string(top_genome[i]) + "\t" + std::to_string(top_kmers[i]) + "\t" +
           (top_genome[i] < genomes.size() ? genomes[top_genome[i]] : std::string(".")) + "\n";
  }
  return out;
}

// ---- --eval-placement ----------------------------------------------------------------------------------------------------------------
static const char* const ASMMAP_JOIN_NAMES[6] = {"none", "inter_genome", "inter_record", "inversion", "relocation", "local"};

std::string asmmap_nga50(const uint64_t* block_length, size_t n, uint64_t target) {
  std::vector<uint64_t> ls(block_length, block_length + n);
  std::sort(ls.begin(), ls.end(), std::greater<uint64_t>());
  unsigned __int128 run = 0;
  for (uint64_t x : ls) {
    run += x;
    if (2 * run >= target) return std::to_string((unsigned long long)x);
  }
  return "NA";
}

std::string asmmap_report(const uint64_t* counts, uint32_t k, uint32_t band, uint32_t relocation, uint32_t min_anchors, const std::vector<std::string>& genomes,
                          const uint64_t* by_genome, const uint64_t* block_length, const uint32_t* block_genome, size_t n_blocks) {
  static const char* const NAMES[ASMMAP_N_COUNTS] = {
      "truth_records", "truth_bases", "truth_invalid", "truth_kmers", "truth_anchors", "truth_repeats", "records", "bases", "invalid", "kmers", "hits", "stray_hits",
      "repeat_hits", "runs", "runs_dropped", "blocks", "block_bases", "breaks_inter_genome", "breaks_inter_record", "breaks_inversion", "breaks_relocation",
      "breaks_local", "contigs_unplaced", "contigs_clean", "contigs_local_only", "contigs_misassembled", "misassembled_bases"};
  auto n = [](uint64_t v) { return std::to_string((unsigned long long)v); };
  std::string out;
  for (size_t i = 0; i < ASMMAP_N_COUNTS; i++) out += std::string("#") + NAMES[i] + "\t" + n(counts[i]) + "\n";
  out += "#k\t" + std::to_string(k) + "\n#band\t" + std::to_string(band) + "\n#relocation\t" + std::to_string(relocation) + "\n#min_anchors\t" +
         std::to_string(min_anchors) + "\n";
  out += "#misassemblies\t" + n(counts[17] + counts[18] + counts[19] + counts[20]) + "\n";
  const uint64_t truth_bases = counts[1], bases = counts[7];
  out += "#NA50\t" + (bases ? asmmap_nga50(block_length, n_blocks, bases) : std::string("NA")) + "\n";
  out += "#NGA50\t" + (truth_bases ? asmmap_nga50(block_length, n_blocks, truth_bases) : std::string("NA")) + "\n";
  out += "#G\tgenome\ttruth_bases\ttruth_anchors\tblocks\tblock_bases\tlongest_block\tNGA50\tanchored\n";
  for (size_t g = 0; g < genomes.size(); g++) {
    const uint64_t* r = by_genome + g * ASMMAP_GENOME_COLS;
    out += "G\t" + genomes[g];
    for (size_t j = 0; j < ASMMAP_GENOME_COLS; j++) out += "\t" + n(r[j]);
    std::vector<uint64_t> own;
    for (size_t i = 0; i < n_blocks; i++)
      if (block_genome[i] == g) own.push_back(block_length[i]);
    char frac[64] = "NA";
    if (r[0] != 0) snprintf(frac, sizeof frac, "%.6f", (double)r[3] / (double)r[0]);
    out += "\t" + (r[0] ? asmmap_nga50(own.data(), own.size(), r[0]) : std::string("NA")) + "\t" + frac + "\n";
  }
  return out;
}

std::string asmmap_block_rows(const std::vector<std::string>& contig_names, const std::vector<std::string>& truth_names, const uint32_t* const cols[9], size_t n) {
  std::string out;
  for (size_t i = 0; i < n; i++) {
    const uint32_t c = cols[0][i], t = cols[1][i], join = cols[8][i];
    out += c < contig_names.size() ? contig_names[c] : std::string("?");
    out += "\t" + std::to_string(cols[3][i]) + "\t" + std::to_string(cols[4][i]) + "\t" + (t < truth_names.size() ? truth_names[t] : std::string("?")) + "\t" +
           std::to_string(cols[5][i]) + "\t" + std::to_string(cols[6][i]) + "\t" + (cols[2][i] ? "-" : "+") + "\t" + std::to_string(cols[7][i]) + "\t" +
           (join < 6 ? ASMMAP_JOIN_NAMES[join] : "?") + "\n";
  }
  return out;
}

std::string asmmap_contig_rows(const std::vector<std::string>& names, const uint64_t* length, const uint32_t* hits, const uint32_t* blocks,
                               const uint32_t* first_block, const uint64_t* block_bases, const uint32_t* worst_join, size_t n) {
  std::string out;
  for (size_t i = 0; i < n; i++) {
    out += i < names.size() ? names[i] : std::string("?");
    out += "\t" + std::to_string((unsigned long long)length[i]) + "\t" + std::to_string(hits[i]) + "\t" + std::to_string(blocks[i]) + "\t" +
           std::to_string(first_block[i]) + "\t" + std::to_string((unsigned long long)block_bases[i]) + "\t" +
           (worst_join[i] < 6 ? ASMMAP_JOIN_NAMES[worst_join[i]] : "?") + "\n";
  }
  return out;
}

// ---- --eval-corrected ----------------------------------------------------------------------------------------------------------------
std::string correval_ratio(bool negative, uint64_t num, uint64_t den) {
  if (den == 0) return "NA";
  const unsigned __int128 q = ((unsigned __int128)num * 2000000u + den) / ((unsigned __int128)den * 2u);  // millionths, half up
  char buf[64];
  snprintf(buf, sizeof buf, "%s%llu.%06llu", negative && q != 0 ? "-" : "", (unsigned long long)(q / 1000000u), (unsigned long long)(q % 1000000u));
  return buf;
}

std::string correval_report(const uint64_t* counts, const uint64_t* cube, const uint64_t* by_qual, const uint64_t* by_pos) {
  static const char* const NAMES[CORREVAL_N_COUNTS] = {
      "truth_lines", "truth_header", "truth_records", "truth_entries", "truth_skipped", "lines", "records", "unknown_read", "scored", "trimmed_records",
      "longer_records", "compared", "kept", "damaged", "fixed", "left", "miscorrected", "ambiguous", "trimmed_error", "trimmed_clean", "extra", "missing",
      "multiple", "clean_kept", "clean_damaged", "fixed_all", "improved", "unchanged", "worse"};
  auto n = [](uint64_t v) { return std::to_string((unsigned long long)v); };
  std::string out;
  for (size_t i = 0; i < CORREVAL_N_COUNTS; i++) out += std::string("#") + NAMES[i] + "\t" + n(counts[i]) + "\n";
  const uint64_t kept = counts[12], damaged = counts[13], fixed = counts[14], left = counts[15], mis = counts[16], trimmed_error = counts[18];
  const unsigned __int128 errors128 = (unsigned __int128)fixed + left + mis + trimmed_error;
  const uint64_t errors = errors128 > UINT64_MAX ? UINT64_MAX : (uint64_t)errors128;   // (sums of positions: far below 2^64)
  const bool neg = damaged > fixed;
  const uint64_t net = neg ? damaged - fixed : fixed - damaged;
  out += "#gain\t" + std::string(neg ? "-" : "") + n(net) + "/" + n(errors) + "\t" + correval_ratio(neg, net, errors) + "\n";
  out += "#sensitivity\t" + n(fixed) + "/" + n(errors) + "\t" + correval_ratio(false, fixed, errors) + "\n";
  const unsigned __int128 clean128 = (unsigned __int128)kept + damaged;
  const uint64_t clean = clean128 > UINT64_MAX ? UINT64_MAX : (uint64_t)clean128;
  out += "#specificity\t" + n(kept) + "/" + n(clean) + "\t" + correval_ratio(false, kept, clean) + "\n";
  auto rows = [&](const char* tag, const char* what, const uint64_t* table, size_t n_rows) {
    out += std::string("#") + tag + "\t" + what + "\tkept\tdamaged\tfixed\tleft\tmiscorrected\n";
    for (size_t r = 0; r < n_rows; r++) {
      const uint64_t* v = table + r * 5;
      if (!(v[0] | v[1] | v[2] | v[3] | v[4])) continue;
      out += std::string(tag) + "\t" + n(r);
      for (int j = 0; j < 5; j++) out += "\t" + n(v[j]);
      out += "\n";
    }
  };
  rows("Q", "quality", by_qual, CORREVAL_N_QUALS);
  rows("P", "position", by_pos, CORREVAL_N_POS);
  out += "#C\ttrue\toriginal\tA\tC\tG\tT\tN\n";
  for (int t = 0; t < 5; t++)
    for (int o = 0; o < 5; o++) {
      out += std::string("C\t") + "ACGTN"[t] + "\t" + "ACGTN"[o];
      for (int c = 0; c < 5; c++) out += "\t" + n(cube[(t * 5 + o) * 5 + c]);
      out += "\n";
    }
  return out;
}

std::string correval_read_rows(const uint64_t* key, const uint32_t* length, const uint32_t* before, const uint32_t* residual, const uint32_t* hits, size_t n) {
  std::string out;
  for (size_t i = 0; i < n; i++) {
    if (hits[i] != 0u && residual[i] == 0u) continue;
    out += std::to_string((unsigned long long)(key[i] >> 1)) + "\t" + std::to_string((unsigned)(key[i] & 1u)) + "\t" + std::to_string(length[i]) + "\t" +
           std::to_string(before[i]) + "\t" + (hits[i] ? std::to_string(residual[i]) : std::string(".")) + "\t" + std::to_string(hits[i]) + "\n";
  }
  return out;
}

// ---- --eval-bins ---------------------------------------------------------------------------------------------------------------------
// calls line(a, b) for every record line text[a, b) of text[0, n): not empty, without its line end, not begun by one of `skip`
template <class F>
static void bineval_lines(const char* text, size_t n, const char* skip, F&& line) {
  for (size_t a = 0; a < n;) {
    size_t nl = a;
    while (nl < n && text[nl] != '\n') nl++;
    size_t b = nl;
    if (nl < n && b > a && text[b - 1] == '\r') b--;
    if (b > a && !strchr(skip, text[a])) line(a, b);
    a = nl + 1;
  }
}

// field `want` (from 1) of text[a, b), "" where the line has fewer
static std::string bineval_field(const char* text, size_t a, size_t b, unsigned want) {
  for (unsigned f = 1;; f++) {
    size_t e = a;
    while (e < b && text[e] != '\t') e++;
    if (f == want) return std::string(text + a, e - a);
    if (e == b) return std::string();
    a = e + 1;
  }
}

void bineval_truth_names(const char* text, size_t n, std::vector<std::string>* contig, std::vector<std::string>* genome) {
  bineval_lines(text, n, "#", [&](size_t a, size_t b) {
    contig->push_back(bineval_field(text, a, b, 1));
    genome->push_back(bineval_field(text, a, b, 8));
  });
}

void bineval_record_bins(const char* text, size_t n, std::vector<std::string>* bin) {
  bineval_lines(text, n, "#@", [&](size_t a, size_t b) { bin->push_back(bineval_field(text, a, b, 2)); });
}

static std::string bineval_frac(double num, double den) {
  char text[64] = "NA";
  if (den != 0.0) snprintf(text, sizeof text, "%.6f", num / den);
  return text;
}

std::string bineval_ari(uint64_t pairs_cells, uint64_t pairs_bins, uint64_t pairs_genomes, uint64_t n) {
  const double all = (double)n * (double)(n ? n - 1 : 0) / 2.0;
  if (all == 0.0) return "NA";
  const double expected = (double)pairs_bins * (double)pairs_genomes / all;
  return bineval_frac((double)pairs_cells - expected, ((double)pairs_bins + (double)pairs_genomes) / 2.0 - expected);
}

std::string bineval_report(const uint64_t* counts, const std::vector<std::string>& genomes, const uint64_t* by_genome, const std::vector<std::string>& bin_names,
                           const uint32_t* contigs, const uint64_t* bases, const uint64_t* none_bases, const uint32_t* top_genome, const uint64_t* top_bases,
                           size_t n_bins) {
  static const char* const NAMES[BINEVAL_N_COUNTS] = {"truth_records", "truth_bases", "truth_none", "records", "unknown_contig", "repeated", "assigned",
                                                      "assigned_bases", "bins", "cells", "sum_top_bases", "sum_best_bases", "pairs_cells", "pairs_bins",
                                                      "pairs_genomes", "bins_c90_x5", "bins_c70_x5", "bins_c50_x5", "bins_c90_x10", "bins_c70_x10", "bins_c50_x10"};
  auto n = [](uint64_t v) { return std::to_string((unsigned long long)v); };
  const size_t G = genomes.size();
  std::string out;
  for (size_t i = 0; i < BINEVAL_N_COUNTS; i++) out += std::string("#") + NAMES[i] + "\t" + n(counts[i]) + "\n";
  const uint64_t truth_bases = counts[1], assigned_bases = counts[7], sum_top = counts[10], sum_best = counts[11];
  uint64_t real_bases = 0, real_assigned = 0;
  for (size_t g = 0; g < G; g++) {
    real_bases += by_genome[g * BINEVAL_GENOME_COLS + 1];
    real_assigned += by_genome[g * BINEVAL_GENOME_COLS + 2];
  }
  out += "#purity\t" + n(sum_top) + "/" + n(assigned_bases) + "\t" + bineval_frac((double)sum_top, (double)assigned_bases) + "\n";
  out += "#completeness\t" + n(sum_best) + "/" + n(real_bases) + "\t" + bineval_frac((double)sum_best, (double)real_bases) + "\n";
  std::string f1 = "NA";
  if (assigned_bases != 0 && real_bases != 0) {
    const double p = (double)sum_top / (double)assigned_bases, c = (double)sum_best / (double)real_bases;
    f1 = bineval_frac(2.0 * p * c, p + c);
  }
  out += "#f1\t" + f1 + "\n";
  out += "#assigned_fraction\t" + n(assigned_bases) + "/" + n(truth_bases) + "\t" + bineval_frac((double)assigned_bases, (double)truth_bases) + "\n";
  out += "#ari_contigs\t" + bineval_ari(counts[12], counts[13], counts[14], real_assigned) + "\n";
  double sum = 0.0;
  uint64_t with = 0;
  for (size_t b = 0; b < n_bins; b++)
    if (bases[b] != 0) { sum += (double)top_bases[b] / (double)bases[b]; with++; }
  out += "#average_purity\t" + bineval_frac(sum, (double)with) + "\n";
  sum = 0.0;
  with = 0;
  for (size_t g = 0; g < G; g++) {
    const uint64_t* r = by_genome + g * BINEVAL_GENOME_COLS;
    if (r[1] != 0) { sum += (double)r[6] / (double)r[1]; with++; }
  }
  out += "#average_completeness\t" + bineval_frac(sum, (double)with) + "\n";
  out += "#G\tgenome\ttruth_contigs\ttruth_bases\tassigned_contigs\tassigned_bases\tbins\tbest_bin\tbest_bases\tcompleteness\n";
  for (size_t g = 0; g <= G; g++) {
    const uint64_t* r = by_genome + g * BINEVAL_GENOME_COLS;
    out += "G\t" + (g < G ? genomes[g] : std::string("."));
    for (size_t j = 0; j < BINEVAL_GENOME_COLS; j++) out += "\t" + n(r[j]);
    out += "\t" + bineval_frac((double)r[6], (double)r[1]) + "\n";
  }
  out += "#B\tbin\tcontigs\tbases\ttop_genome\ttop_bases\tnone_bases\tpurity\tcompleteness\n";
  for (size_t b = 0; b < n_bins; b++) {
    const bool top = top_genome[b] < G;
    out += "B\t" + (b < bin_names.size() ? bin_names[b] : std::string("?")) + "\t" + std::to_string(contigs[b]) + "\t" + n(bases[b]) + "\t" +
           (top ? genomes[top_genome[b]] : std::string(".")) + "\t" + n(top_bases[b]) + "\t" + n(none_bases[b]) + "\t" +
           bineval_frac((double)top_bases[b], (double)bases[b]) + "\t" +
           (top ? bineval_frac((double)top_bases[b], (double)by_genome[top_genome[b] * BINEVAL_GENOME_COLS + 1]) : std::string("NA")) + "\n";
  }
  return out;
}

std::string bineval_cell_rows(const std::vector<std::string>& bin_names, const std::vector<std::string>& genomes, const uint32_t* bin, const uint32_t* genome,
                              const uint32_t* contigs, const uint64_t* bases, size_t n) {
  std::string out;
  for (size_t i = 0; i < n; i++)
    out += (bin[i] < bin_names.size() ? bin_names[bin[i]] : std::string("?")) + "\t" + (genome[i] < genomes.size() ? genomes[genome[i]] : std::string(".")) + "\t" +
           std::to_string(contigs[i]) + "\t" + std::to_string((unsigned long long)bases[i]) + "\n";
  return out;
}

std::string bineval_contig_rows(const std::vector<std::string>& names, const std::vector<std::string>& genomes, const std::vector<std::string>& bin_names,
                                const uint32_t* genome, const uint64_t* length, const uint32_t* bin, const uint32_t* records, size_t n) {
  std::string out;
  for (size_t i = 0; i < n; i++)
    out += (i < names.size() ? names[i] : std::string("?")) + "\t" + std::to_string((unsigned long long)length[i]) + "\t" +
           (genome[i] < genomes.size() ? genomes[genome[i]] : std::string(".")) + "\t" + (bin[i] < bin_names.size() ? bin_names[bin[i]] : std::string(".")) + "\t" +
           std::to_string(records[i]) + "\n";
  return out;
}

// ---- a file in pieces ------------------------------------------------------------------------------------------------------------------
size_t piece_cut(const uint8_t* p, size_t have, PieceCut rule) {
  size_t cut = 0;
  switch (rule.kind) {
    case PieceCut::Newline:
      for (cut = have; cut > 0 && p[cut - 1] != '\n';) cut--;
      break;
    case PieceCut::Fasta:
      for (cut = have; cut > 1 && !(p[cut - 1] == '>' && p[cut - 2] == '\n');) cut--;
      cut = cut > 1 ? cut - 1 : 0;  // in front of the '>'
      break;
    case PieceCut::Record:
      for (size_t i = 0, lines = 0; i < have; i++)
        if (p[i] == '\n' && ++lines % rule.lines == 0) cut = i + 1;
      break;
  }
  return cut;
}

PieceReader::End PieceReader::next(const uint8_t** p, size_t* n) {
  if (cut_ > 0) {  // the open last line or record of the piece before moves to the front
    memmove(buf_.data(), buf_.data() + cut_, have_ - cut_);
    have_ -= cut_;
    cut_ = 0;
  }
  while (!eof_) {
    if (buf_.size() < have_ + piece_) buf_.resize(have_ + piece_);
    const size_t got = fread(buf_.data() + have_, 1, piece_, f_);
    if (got < piece_) {
      if (ferror(f_)) return CannotRead;
      eof_ = true;
    }
    have_ += got;
    const size_t cut = eof_ ? have_ : piece_cut(buf_.data(), have_, rule_);
    if (cut == 0) {  // longer than the buffer: read on (or the file's end with nothing left)
      if (!eof_ && rule_.kind == PieceCut::Fasta && have_ > max_) return TooLong;
      continue;
    }
    if (cut > max_) return TooLong;
    cut_ = cut;
    *p = buf_.data();
    *n = cut;
    return Piece;
  }
  return Done;
}

// ---- --eval-classified ---------------------------------------------------------------------------------------------------------------
static const char* const TAXEVAL_RANK_NAMES[TAXEVAL_RANKS + 1] = {"no_rank", "domain", "phylum", "class", "order", "family", "genus", "species", "strain"};

uint8_t taxeval_rank_code(const std::string& name) {
  if (name == "superkingdom") return 1;
  for (size_t r = 1; r <= TAXEVAL_RANKS; r++)
    if (name == TAXEVAL_RANK_NAMES[r]) return (uint8_t)r;
  return 0;
}

const char* taxeval_rank_name(uint32_t code) { return TAXEVAL_RANK_NAMES[code <= TAXEVAL_RANKS ? code : 0]; }

// the fields of text[a, b): cut at "\t|\t" where the line holds one (a trailing "\t|" dropped), at tabs otherwise
static std::vector<std::string> taxeval_fields(const char* text, size_t a, size_t b) {
  std::string line(text + a, b - a);
  if (!line.empty() && line.back() == '\r') line.pop_back();
  std::vector<std::string> out;
  const bool dmp = line.find("\t|\t") != std::string::npos;
  if (dmp && line.size() >= 2 && line.compare(line.size() - 2, 2, "\t|") == 0) line.resize(line.size() - 2);
  const std::string sep = dmp ? "\t|\t" : "\t";
  for (size_t at = 0;;) {
    const size_t e = line.find(sep, at);
    out.push_back(line.substr(at, e == std::string::npos ? std::string::npos : e - at));
    if (e == std::string::npos) break;
    at = e + sep.size();
  }
  return out;
}

static bool taxeval_taxid(const std::string& s, uint32_t* out) {
  if (s.empty() || s.size() > 10) return false;
  uint64_t v = 0;
  for (char c : s) {
    if (c < '0' || c > '9') return false;
    v = v * 10 + (uint64_t)(c - '0');
  }
  if (v > 0xffffffffull) return false;
  *out = (uint32_t)v;
  return true;
}

bool taxeval_parse_nodes(const char* text, size_t n, std::vector<uint32_t>* taxid, std::vector<uint32_t>* parent, std::vector<uint8_t>* rank, std::string* err) {
  size_t line_no = 0;
  for (size_t a = 0; a < n;) {
    size_t b = a;
    while (b < n && text[b] != '\n') b++;
    line_no++;
    if (b > a && !(b - a == 1 && text[a] == '\r')) {
      const std::vector<std::string> f = taxeval_fields(text, a, b);
      uint32_t t = 0, p = 0;
      if (f.size() < 3 || !taxeval_taxid(f[0], &t) || !taxeval_taxid(f[1], &p)) {
        *err = "line " + std::to_string(line_no) + " is not 'taxid | parent | rank'";
        return false;
      }
      taxid->push_back(t);
      parent->push_back(p);
      rank->push_back(taxeval_rank_code(f[2]));
    }
    a = b + 1;
  }
  return true;
}

bool taxeval_parse_map(const char* text, size_t n, std::vector<std::string>* genome_id, std::vector<uint32_t>* taxid, std::string* err) {
  size_t line_no = 0;
  bool first = true;  // the first line that is not empty may be a header
  for (size_t a = 0; a < n;) {
    size_t b = a;
    while (b < n && text[b] != '\n') b++;
    line_no++;
    if (b > a && !(b - a == 1 && text[a] == '\r')) {
      std::string line(text + a, b - a);
      if (line.back() == '\r') line.pop_back();
      const size_t tab = line.find('\t');
      const size_t e = tab == std::string::npos ? tab : line.find('\t', tab + 1);
      uint32_t t = 0;
      const bool ok = tab != std::string::npos && tab > 0 && taxeval_taxid(line.substr(tab + 1, e == std::string::npos ? e : e - tab - 1), &t);
      if (!ok && !(first && tab != std::string::npos)) {
        *err = "line " + std::to_string(line_no) + " is not 'genome_id <tab> taxid'";
        return false;
      }
      if (ok) {
        genome_id->push_back(line.substr(0, tab));
        taxid->push_back(t);
      }
      first = false;
    }
    a = b + 1;
  }
  return true;
}

static std::string taxeval_ratio(uint64_t num, uint64_t den) {
  if (den == 0) return "NA";
  char text[64];
  snprintf(text, sizeof text, "%.6f", (double)num / (double)den);
  return text;
}

// precision, sensitivity and F1 of one row of five class counts
static std::string taxeval_prf(const uint64_t* k) {
  const uint64_t scored = k[1] + k[2] + k[3] + k[4], cw = k[4] + k[2];
  std::string f1 = "NA";
  if (cw != 0 && scored != 0) {
    const double p = (double)k[4] / (double)cw, s = (double)k[4] / (double)scored;
    if (p + s != 0.0) {
      char text[64];
      snprintf(text, sizeof text, "%.6f", 2.0 * p * s / (p + s));
      f1 = text;
    }
  }
  return taxeval_ratio(k[4], cw) + "\t" + taxeval_ratio(k[4], scored) + "\t" + f1;
}

std::string taxeval_report(const uint64_t* counts, const uint64_t* by_rank, const uint64_t* reads_by_rank, const uint8_t* rank_code, const uint64_t* true_sum,
                           const uint64_t* called_sum, size_t n_nodes) {
  static const char* const NAMES[TAXEVAL_N_COUNTS] = {"truth_lines", "truth_header", "truth_entries", "truth_paired", "lines", "header", "records", "unknown_read",
                                                      "unclassified", "unknown_taxon", "scored", "missing", "multiple"};
  static const char* const CLASS[TAXEVAL_CLASSES] = {"absent", "unclassified", "wrong", "above", "correct"};
  auto n = [](uint64_t v) { return std::to_string((unsigned long long)v); };
  std::string out;
  for (size_t i = 0; i < TAXEVAL_N_COUNTS; i++) out += std::string("#") + NAMES[i] + "\t" + n(counts[i]) + "\n";
  out += "#R\trank\tname";
  for (const char* w : {"records", "reads"})
    for (size_t k = 0; k < TAXEVAL_CLASSES; k++) out += std::string("\t") + w + "_" + CLASS[k];
  out += "\n";
  for (size_t r = 0; r < TAXEVAL_RANKS; r++) {
    out += "R\t" + std::to_string(r + 1) + "\t" + TAXEVAL_RANK_NAMES[r + 1];
    for (size_t k = 0; k < TAXEVAL_CLASSES; k++) out += "\t" + n(by_rank[r * TAXEVAL_CLASSES + k]);
    for (size_t k = 0; k < TAXEVAL_CLASSES; k++) out += "\t" + n(reads_by_rank[r * TAXEVAL_CLASSES + k]);
    out += "\n";
  }
  out += "#P\trank\tname\trecords_precision\trecords_sensitivity\trecords_f1\treads_precision\treads_sensitivity\treads_f1\n";
  for (size_t r = 0; r < TAXEVAL_RANKS; r++)
    out += "P\t" + std::to_string(r + 1) + "\t" + TAXEVAL_RANK_NAMES[r + 1] + "\t" + taxeval_prf(by_rank + r * TAXEVAL_CLASSES) + "\t" +
           taxeval_prf(reads_by_rank + r * TAXEVAL_CLASSES) + "\n";
  out += "#A\trank\tname\tnodes\tl1_distance\n";
  for (size_t r = 1; r <= TAXEVAL_RANKS; r++) {
    uint64_t st = 0, sc = 0, nodes = 0;
    for (size_t i = 0; i < n_nodes; i++)
      if (rank_code[i] == r) { st += true_sum[i]; sc += called_sum[i]; nodes++; }
    double l1 = 0.0;
    if (st != 0 && sc != 0)
      for (size_t i = 0; i < n_nodes; i++)
        if (rank_code[i] == r) l1 += fabs((double)true_sum[i] / (double)st - (double)called_sum[i] / (double)sc);
    char text[64] = "NA";
    if (st != 0 && sc != 0) snprintf(text, sizeof text, "%.6f", l1);
    out += "A\t" + std::to_string(r) + "\t" + TAXEVAL_RANK_NAMES[r] + "\t" + n(nodes) + "\t" + text + "\n";
  }
  return out;
}

std::string taxeval_read_rows(const std::vector<std::string>& genome_ids, const std::vector<uint32_t>& genome_has, const uint64_t* id, const uint32_t* genome,
                              const uint32_t* mates, const uint32_t* seen, const uint32_t* hits, size_t n) {
  std::string out;
  for (size_t i = 0; i < n; i++) {
    const uint32_t g = genome[i];
    out += std::to_string((unsigned long long)id[i]) + "\t" + (g < genome_ids.size() ? genome_ids[g] : std::string("?")) + "\t" + std::to_string(mates[i]) + "\t" +
           std::to_string(hits[i]);
    const uint32_t has = g < genome_has.size() ? genome_has[g] : 0u;
    for (size_t r = 0; r < TAXEVAL_RANKS; r++) {
      const uint32_t nib = (seen[i] >> (4 * r)) & 15u;
      const uint32_t best = hits[i] == 0 ? (has >> r) & 1u : nib ? 32u - (uint32_t)__builtin_clz(nib) : 0u;
      out += "\t" + std::to_string(best);
    }
    out += "\n";
  }
  return out;
}

std::string taxeval_taxa_rows(const uint32_t* taxid, const uint8_t* rank_code, const uint64_t* true_sum, const uint64_t* called_sum, const uint64_t* both_sum,
                              size_t n_nodes) {
  std::string out;
  for (size_t i = 0; i < n_nodes; i++) {
    if (true_sum[i] == 0 && called_sum[i] == 0 && both_sum[i] == 0) continue;
    out += std::to_string(taxid[i]) + "\t" + taxeval_rank_name(rank_code[i]) + "\t" + std::to_string((unsigned long long)true_sum[i]) + "\t" +
           std::to_string((unsigned long long)called_sum[i]) + "\t" + std::to_string((unsigned long long)both_sum[i]) + "\t" +
           taxeval_ratio(both_sum[i], called_sum[i]) + "\t" + taxeval_ratio(both_sum[i], true_sum[i]) + "\n";
  }
  return out;
}

static bool parse_u64(const std::string& s, uint64_t max, uint64_t* out) {
  if (s.empty()) return false;
  char* end = nullptr;
  unsigned long long v = strtoull(s.c_str(), &end, 10);
  if (*end != 0 || s[0] == '-' || v > max) return false;
  *out = v;
  return true;
}

bool parse_cli_args(int argc, const char* const* argv, CliArgs* a, std::string* err, bool* help) {
  *help = false;
  std::string first_other, first_not_eval, first_eval, first_not_ovl, first_ovl, first_not_vcf, first_vcf, first_not_tax, first_tax, first_not_asm, first_asm, first_not_bin, first_bin, first_not_corr, first_corr, first_not_place, first_place;
  for (int i = 1; i < argc; i++) {
    std::string arg = argv[i], val;
    bool has_val = false;
    size_t eq = arg.find('=');
    if (arg.rfind("--", 0) == 0 && eq != std::string::npos) { val = arg.substr(eq + 1); arg = arg.substr(0, eq); has_val = true; }
    auto need = [&](std::string* dst) -> bool {
      if (has_val) { *dst = val; return true; }
      if (i + 1 >= argc) { *err = "a value is required for '" + arg + "'"; return false; }
      *dst = argv[++i];
      return true;
    };
    std::string v;
    uint64_t u;
    // a value in [lo, max] into u; whatever is wrong with it, a missing value included, is the one message
    auto uint = [&](uint64_t lo, uint64_t max, const char* hint = "") -> bool {
      if (need(&v) && parse_u64(v, max, &u) && u >= lo) return true;
      *err = "invalid value for " + arg + hint;
      return false;
    };
    auto file = [&](std::string* dst) -> bool {  // a file name that is not empty
      if (need(dst) && dst->empty()) *err = "a file name is required for '" + arg + "'";
      return err->empty();
    };
    if (arg == "--help" || arg == "-h") { *help = true; return true; }
    if (first_other.empty() && arg != "--fit-from-sam" && arg != "--fit-model" && arg != "--fit-k" && arg != "--fit-max-alt" &&
        arg != "--single-reads" && arg != "--device")
      first_other = arg;  // what --fit-from-sam does not take
    const bool eval_flag = arg == "--eval-sam" || arg == "--eval-truth" || arg == "--eval-report" || arg == "--eval-reads" || arg == "--eval-min-overlap";
    if (eval_flag && first_eval.empty()) first_eval = arg;
    if (!eval_flag && arg != "--device" && first_not_eval.empty()) first_not_eval = arg;  // what --eval-sam does not take
    const bool ovl_flag = arg == "--eval-overlaps" || arg == "--eval-overlaps-truth" || arg == "--eval-overlaps-report" || arg == "--eval-overlaps-pairs" ||
                          arg == "--eval-overlaps-min-pct";
    if (ovl_flag && first_ovl.empty()) first_ovl = arg;
    if (!ovl_flag && arg != "--device" && first_not_ovl.empty()) first_not_ovl = arg;  // what --eval-overlaps does not take
    const bool vcf_flag = arg == "--eval-vcf" || arg == "--eval-vcf-truth" || arg == "--eval-vcf-report" || arg == "--eval-vcf-sites" || arg == "--eval-vcf-filtered";
    if (vcf_flag && first_vcf.empty()) first_vcf = arg;
    if (!vcf_flag && arg != "--device" && first_not_vcf.empty()) first_not_vcf = arg;  // what --eval-vcf does not take
    const bool tax_flag = arg == "--eval-classified" || arg == "--eval-classified-truth" || arg == "--eval-taxonomy" || arg == "--eval-genome-taxa" ||
                          arg == "--eval-classified-report" || arg == "--eval-classified-reads" || arg == "--eval-classified-taxa";
    if (tax_flag && first_tax.empty()) first_tax = arg;
    if (!tax_flag && arg != "--device" && first_not_tax.empty()) first_not_tax = arg;  // what --eval-classified does not take
    const bool asm_flag = arg == "--eval-assembly" || arg == "--eval-assembly-truth" || arg == "--eval-assembly-report" || arg == "--eval-assembly-contigs" ||
                          arg == "--eval-assembly-k";
    if (asm_flag && first_asm.empty()) first_asm = arg;
    if (!asm_flag && arg != "--device" && first_not_asm.empty()) first_not_asm = arg;  // what --eval-assembly does not take
    const bool place_flag = arg.compare(0, 16, "--eval-placement") == 0;
    if (place_flag && first_place.empty()) first_place = arg;
    if (!place_flag && arg != "--device" && first_not_place.empty()) first_not_place = arg;  // what --eval-placement does not take
    const bool bin_flag = arg == "--eval-bins" || arg == "--eval-bins-truth" || arg == "--eval-bins-report" || arg == "--eval-bins-bins" || arg == "--eval-bins-contigs";
    if (bin_flag && first_bin.empty()) first_bin = arg;
    if (!bin_flag && arg != "--device" && first_not_bin.empty()) first_not_bin = arg;  // what --eval-bins does not take
    const bool corr_flag = arg == "--eval-corrected" || arg == "--eval-corrected-truth" || arg == "--eval-corrected-report" || arg == "--eval-corrected-reads" ||
                           arg == "--eval-corrected-fasta";
    if (corr_flag && first_corr.empty()) first_corr = arg;
    if (!corr_flag && arg != "--device" && first_not_corr.empty()) first_not_corr = arg;  // what --eval-corrected does not take
    if (arg == "--fit-from-sam") { if (!file(&a->fit_from_sam)) return false; }
    else if (arg == "--eval-corrected") { if (!file(&a->eval_corrected)) return false; }
    else if (arg == "--eval-corrected-truth") { if (!file(&a->eval_corrected_truth)) return false; }
    else if (arg == "--eval-corrected-report") { if (!file(&a->eval_corrected_report)) return false; }
    else if (arg == "--eval-corrected-reads") { if (!file(&a->eval_corrected_reads)) return false; }
    else if (arg == "--eval-corrected-fasta") a->eval_corrected_fasta = true;
    else if (arg == "--eval-assembly") { if (!file(&a->eval_assembly)) return false; }
    else if (arg == "--eval-bins") { if (!file(&a->eval_bins)) return false; }
    else if (arg == "--eval-bins-truth") { if (!file(&a->eval_bins_truth)) return false; }
    else if (arg == "--eval-bins-report") { if (!file(&a->eval_bins_report)) return false; }
    else if (arg == "--eval-bins-bins") { if (!file(&a->eval_bins_bins)) return false; }
    else if (arg == "--eval-bins-contigs") { if (!file(&a->eval_bins_contigs)) return false; }
    else if (arg == "--eval-assembly-truth") { if (!file(&a->eval_assembly_truth)) return false; }
    else if (arg == "--eval-assembly-report") { if (!file(&a->eval_assembly_report)) return false; }
    else if (arg == "--eval-assembly-contigs") { if (!file(&a->eval_assembly_contigs)) return false; }
    else if (arg == "--eval-assembly-k") {
      if (!uint(15, 31)) return false;
      if (u % 2 == 0) { *err = "invalid value '" + v + "' for '--eval-assembly-k': k is odd"; return false; }
      a->eval_assembly_k = (uint32_t)u;
    }
    else if (arg == "--eval-placement") { if (!file(&a->eval_placement)) return false; }
    else if (arg == "--eval-placement-truth") { if (!file(&a->eval_placement_truth)) return false; }
    else if (arg == "--eval-placement-report") { if (!file(&a->eval_placement_report)) return false; }
    else if (arg == "--eval-placement-blocks") { if (!file(&a->eval_placement_blocks)) return false; }
    else if (arg == "--eval-placement-contigs") { if (!file(&a->eval_placement_contigs)) return false; }
    else if (arg == "--eval-placement-k") {
      if (!uint(15, 31)) return false;
      if (u % 2 == 0) { *err = "invalid value '" + v + "' for '--eval-placement-k': k is odd"; return false; }
      a->eval_placement_k = (uint32_t)u;
    }
    else if (arg == "--eval-placement-band") { if (!uint(0, 0x7fffffffull)) return false; a->eval_placement_band = (uint32_t)u; }
    else if (arg == "--eval-placement-relocation") { if (!uint(0, 0x7fffffffull)) return false; a->eval_placement_relocation = (uint32_t)u; }
    else if (arg == "--eval-placement-min-anchors") { if (!uint(1, 0xffffffffull)) return false; a->eval_placement_min_anchors = (uint32_t)u; }
    else if (arg == "--single-reads") a->single_reads = true;
    else if (arg == "--genome") { if (!need(&v)) return false; a->genome.push_back(v); }
    else if (arg == "--genome-file") { if (!need(&v)) return false; a->genome_file = v; }
    else if (arg == "--output") { if (!need(&v)) return false; a->output = v; }
    else if (arg == "--num-reads") { if (!uint(0, UINT64_MAX)) return false; a->num_reads = u; }
    else if (arg == "--read-length") { if (!uint(0, 65535)) return false; a->read_length = (uint16_t)u; }
    else if (arg == "--read-length-std") { if (!need(&v)) return false; a->read_length_std = atof(v.c_str()); }
    else if (arg == "--insert-size") { if (!uint(0, 65535)) return false; a->insert_size = (uint16_t)u; }
    else if (arg == "--mean-phred-score") { if (!uint(0, 255)) return false; a->mean_phred_score = (uint8_t)u; }
    else if (arg == "--error-profile") {
      if (!need(&v)) return false;
      if (v == "minimal-short") a->error_profile = ErrorProfileKind::MinimalShort;
      else if (v == "minimal-long") a->error_profile = ErrorProfileKind::MinimalLong;
      else if (v == "perfect-short") a->error_profile = ErrorProfileKind::PerfectShort;
      else if (v == "perfect-long") a->error_profile = ErrorProfileKind::PerfectLong;
      else if (v == "custom-short") a->error_profile = ErrorProfileKind::CustomShort;
      else if (v == "custom-long") a->error_profile = ErrorProfileKind::CustomLong;  // extension, see usage()
      else { *err = "invalid value '" + v + "' for '--error-profile'"; return false; }
    } else if (arg == "--abundance-profile") {
      if (!need(&v)) return false;
      if (v == "exact") a->abundance_profile = AbundanceProfileKind::Exact;
      else if (v == "uniform") a->abundance_profile = AbundanceProfileKind::Uniform;
      else if (v == "custom") a->abundance_profile = AbundanceProfileKind::Custom;
      else { *err = "invalid value '" + v + "' for '--abundance-profile'"; return false; }
    }
    else if (arg == "--custom-profile") { if (!need(&v)) return false; a->custom_profile = v; }
    else if (arg == "--with-ani") {  // a percentage in plain decimal notation: digits, at most one point
      const bool plain = need(&v) && v.find_first_not_of("0123456789.") == std::string::npos && v.find_first_of("0123456789") != std::string::npos &&
                         std::count(v.begin(), v.end(), '.') <= 1;
      const double pct = plain ? strtod(v.c_str(), nullptr) : 0.0;
      if (!(pct >= 25.0 && pct <= 100.0)) { *err = "invalid value for --with-ani"; return false; }
      a->with_ani = pct;
    }
    else if (arg == "--read-header-format") { if (!need(&v)) return false; a->read_header_format = v; }
    else if (arg == "--seed") { if (!uint(0, UINT64_MAX)) return false; a->seed = u; }
    else if (arg == "--size-adjusted") a->size_adjusted = true;
    else if (arg == "--contiguous") a->contiguous = true;
    else if (arg == "--host-fastq") a->host_fastq = true;
    else if (arg == "--host-normalize") a->host_normalize = true;
    else if (arg == "--truth") { if (!file(&a->truth)) return false; }
    else if (arg == "--sam") { if (!file(&a->sam)) return false; }
    else if (arg == "--sam-sorted") a->sam_sorted = true;
    else if (arg == "--bam") { if (!file(&a->bam)) return false; }
    else if (arg == "--bam-sorted") a->bam_sorted = true;
    else if (arg == "--bam-index") { if (!file(&a->bam_index)) return false; }
    else if (arg == "--overlaps") { if (!file(&a->overlaps)) return false; }
    else if (arg == "--min-overlap") { if (!uint(1, UINT64_MAX, " (at least 1)")) return false; a->min_overlap = u; }
    else if (arg == "--stats") { if (!file(&a->stats)) return false; }
    else if (arg == "--fit-model") { if (!file(&a->fit_model)) return false; }
    else if (arg == "--fit-k") { if (!uint(3, 10, " (3 .. 10)")) return false; a->fit_k = (uint32_t)u; }
    else if (arg == "--eval-sam") { if (!file(&a->eval_sam)) return false; }
    else if (arg == "--eval-truth") { if (!file(&a->eval_truth)) return false; }
    else if (arg == "--eval-report") { if (!file(&a->eval_report)) return false; }
    else if (arg == "--eval-reads") { if (!file(&a->eval_reads)) return false; }
    else if (arg == "--eval-min-overlap") { if (!uint(1, 100, " (1 .. 100)")) return false; a->eval_min_overlap = (uint32_t)u; }
    else if (arg == "--eval-overlaps") { if (!file(&a->eval_overlaps)) return false; }
    else if (arg == "--eval-overlaps-truth") { if (!file(&a->eval_overlaps_truth)) return false; }
    else if (arg == "--eval-overlaps-report") { if (!file(&a->eval_overlaps_report)) return false; }
    else if (arg == "--eval-overlaps-pairs") { if (!file(&a->eval_overlaps_pairs)) return false; }
    else if (arg == "--eval-overlaps-min-pct") { if (!uint(1, 100, " (1 .. 100)")) return false; a->eval_overlaps_min_pct = (uint32_t)u; }
    else if (arg == "--eval-vcf") { if (!file(&a->eval_vcf)) return false; }
    else if (arg == "--eval-vcf-truth") { if (!file(&a->eval_vcf_truth)) return false; }
    else if (arg == "--eval-vcf-report") { if (!file(&a->eval_vcf_report)) return false; }
    else if (arg == "--eval-vcf-sites") { if (!file(&a->eval_vcf_sites)) return false; }
    else if (arg == "--eval-vcf-filtered") a->eval_vcf_filtered = true;
    else if (arg == "--eval-classified") { if (!file(&a->eval_classified)) return false; }
    else if (arg == "--eval-classified-truth") { if (!file(&a->eval_classified_truth)) return false; }
    else if (arg == "--eval-taxonomy") { if (!file(&a->eval_taxonomy)) return false; }
    else if (arg == "--eval-genome-taxa") { if (!file(&a->eval_genome_taxa)) return false; }
    else if (arg == "--eval-classified-report") { if (!file(&a->eval_classified_report)) return false; }
    else if (arg == "--eval-classified-reads") { if (!file(&a->eval_classified_reads)) return false; }
    else if (arg == "--eval-classified-taxa") { if (!file(&a->eval_classified_taxa)) return false; }
    else if (arg == "--fit-max-alt") { if (!uint(1, UINT32_MAX, " (at least 1)")) return false; a->fit_max_alt = (uint32_t)u; }
    else if (arg == "--depth") { if (!file(&a->depth)) return false; }
    else if (arg == "--depth-track") { if (!file(&a->depth_track)) return false; }
    else if (arg == "--strain-sites") { if (!file(&a->strain_sites)) return false; }
    else if (arg == "--strain-vcf") { if (!file(&a->strain_vcf)) return false; }
    else if (arg == "--gold-assembly") { if (!file(&a->gold_assembly)) return false; }
    else if (arg == "--gold-regions") { if (!file(&a->gold_regions)) return false; }
    else if (arg == "--gold-min-depth") { if (!uint(1, UINT32_MAX, " (at least 1)")) return false; a->gold_min_depth = (uint32_t)u; }
    else if (arg == "--gold-min-length") { if (!uint(1, UINT64_MAX, " (at least 1)")) return false; a->gold_min_length = u; }
    else if (arg == "--depth-window") { if (!uint(1, (1u << 30) - 1, " (1 .. 2^30 - 1)")) return false; a->depth_window = (uint32_t)u; }
    else if (arg == "--device-chunk-reads") { if (!uint(1, UINT64_MAX)) return false; a->device_chunk_reads = u; }
    else if (arg == "--devices") {
      if (!need(&v)) return false;
      a->devices.clear();
      size_t pos = 0;
      while (pos <= v.size()) {
        const size_t comma = std::min(v.find(',', pos), v.size());
        if (!parse_u64(v.substr(pos, comma - pos), 1023, &u)) { *err = "invalid value for --devices (a comma-separated list of device ordinals)"; return false; }
        a->devices.push_back((int)u);
        pos = comma + 1;
      }
      if (a->devices.empty() || a->devices.size() > 64) { *err = "invalid value for --devices"; return false; }
    }
    else if (arg == "--device") { if (!uint(0, 1023)) return false; a->device = (int)u; }
    else if (arg == "--gamma") {
      if (!need(&v)) return false;
      float m = 0, s = 0;
      if (sscanf(v.c_str(), "%f,%f", &m, &s) != 2 || !(m > 0) || !(s > 0)) { *err = "--gamma expects mean,std"; return false; }
      a->gamma = std::make_pair(m, s);
    }
    else if (arg == "--per-read-lengths") a->per_read_lengths = true;
    else if (arg == "--rng") {
      if (!need(&v)) return false;
      if (v == "philox") { a->rng_philox = true; a->rng_philox_full = false; }
      else if (v == "philox-full") { a->rng_philox = true; a->rng_philox_full = true; }
      else if (v == "reference") { a->rng_philox = false; a->rng_philox_full = false; }
      else { *err = "invalid value for --rng (reference, philox, philox-full)"; return false; }
    }
    else if (arg == "--uniform-start") a->uniform_start = true;
    else { *err = "Found argument '" + arg + "' which wasn't expected"; return false; }
  }
  if (!a->fit_from_sam.empty()) {  // no simulation: nothing of a run is asked for, and none of its flags is taken
    if (!a->devices.empty()) { *err = "--fit-from-sam does not combine with --devices: use --device"; return false; }
    if (!first_other.empty()) {
      *err = "--fit-from-sam runs no simulation: it takes only --fit-model, --fit-k, --fit-max-alt, --single-reads and --device ('" + first_other + "' given)";
      return false;
    }
    if (a->fit_model.empty()) { *err = "--fit-from-sam needs --fit-model"; return false; }
    return true;
  }
  if (!first_eval.empty()) {  // no simulation either: a mode of its own beside --fit-from-sam
    if (a->eval_sam.empty()) { *err = first_eval + " needs --eval-sam"; return false; }
    if (!first_not_eval.empty()) {
      *err = "--eval-sam runs no simulation: it takes only --eval-truth, --eval-report, --eval-reads, --eval-min-overlap and --device ('" + first_not_eval +
             "' given)";
      return false;
    }
    if (a->eval_truth.empty()) { *err = "--eval-sam needs --eval-truth"; return false; }
    if (a->eval_report.empty()) { *err = "--eval-sam needs --eval-report"; return false; }
    return true;
  }
  if (!first_ovl.empty()) {  // the third mode without a simulation
    if (a->eval_overlaps.empty()) { *err = first_ovl + " needs --eval-overlaps"; return false; }
    if (!first_not_ovl.empty()) {
      *err = "--eval-overlaps runs no simulation: it takes only --eval-overlaps-truth, --eval-overlaps-report, --eval-overlaps-pairs, "
             "--eval-overlaps-min-pct and --device ('" + first_not_ovl + "' given)";
      return false;
    }
    if (a->eval_overlaps_truth.empty()) { *err = "--eval-overlaps needs --eval-overlaps-truth"; return false; }
    if (a->eval_overlaps_report.empty()) { *err = "--eval-overlaps needs --eval-overlaps-report"; return false; }
    return true;
  }
  if (!first_vcf.empty()) {  // the fourth mode without a simulation
    if (a->eval_vcf.empty()) { *err = first_vcf + " needs --eval-vcf"; return false; }
    if (!first_not_vcf.empty()) {
      *err = "--eval-vcf runs no simulation: it takes only --eval-vcf-truth, --eval-vcf-report, --eval-vcf-sites, --eval-vcf-filtered and --device ('" +
             first_not_vcf + "' given)";
      return false;
    }
    if (a->eval_vcf_truth.empty()) { *err = "--eval-vcf needs --eval-vcf-truth"; return false; }
    if (a->eval_vcf_report.empty()) { *err = "--eval-vcf needs --eval-vcf-report"; return false; }
    return true;
  }
  if (!first_tax.empty()) {  // the fifth mode without a simulation
    if (a->eval_classified.empty()) { *err = first_tax + " needs --eval-classified"; return false; }
    if (!first_not_tax.empty()) {
      *err = "--eval-classified runs no simulation: it takes only --eval-classified-truth, --eval-taxonomy, --eval-genome-taxa, --eval-classified-report, "
             "--eval-classified-reads, --eval-classified-taxa and --device ('" + first_not_tax + "' given)";
      return false;
    }
    if (a->eval_classified_truth.empty()) { *err = "--eval-classified needs --eval-classified-truth"; return false; }
    if (a->eval_taxonomy.empty()) { *err = "--eval-classified needs --eval-taxonomy"; return false; }
    if (a->eval_genome_taxa.empty()) { *err = "--eval-classified needs --eval-genome-taxa"; return false; }
    if (a->eval_classified_report.empty()) { *err = "--eval-classified needs --eval-classified-report"; return false; }
    return true;
  }
  if (!first_asm.empty()) {  // the sixth mode without a simulation
    if (a->eval_assembly.empty()) { *err = first_asm + " needs --eval-assembly"; return false; }
    if (!first_not_asm.empty()) {
      *err = "--eval-assembly runs no simulation: it takes only --eval-assembly-truth, --eval-assembly-report, --eval-assembly-contigs, --eval-assembly-k "
             "and --device ('" + first_not_asm + "' given)";
      return false;
    }
    if (a->eval_assembly_truth.empty()) { *err = "--eval-assembly needs --eval-assembly-truth"; return false; }
    if (a->eval_assembly_report.empty()) { *err = "--eval-assembly needs --eval-assembly-report"; return false; }
    return true;
  }
  if (!first_place.empty()) {  // a mode without a simulation beside --eval-assembly: the same two files, placed instead of counted
    if (a->eval_placement.empty()) { *err = first_place + " needs --eval-placement"; return false; }
    if (!first_not_place.empty()) {
      *err = "--eval-placement runs no simulation: it takes only --eval-placement-truth, --eval-placement-report, --eval-placement-blocks, "
             "--eval-placement-contigs, --eval-placement-k, --eval-placement-band, --eval-placement-relocation, --eval-placement-min-anchors and --device ('" +
             first_not_place + "' given)";
      return false;
    }
    if (a->eval_placement_truth.empty()) { *err = "--eval-placement needs --eval-placement-truth"; return false; }
    if (a->eval_placement_report.empty()) { *err = "--eval-placement needs --eval-placement-report"; return false; }
    if (a->eval_placement_band > a->eval_placement_relocation) {
      *err = "--eval-placement-band " + std::to_string(a->eval_placement_band) + " is above --eval-placement-relocation " + std::to_string(a->eval_placement_relocation);
      return false;
    }
    return true;
  }
  if (!first_bin.empty()) {  // the seventh mode without a simulation
    if (a->eval_bins.empty()) { *err = first_bin + " needs --eval-bins"; return false; }
    if (!first_not_bin.empty()) {
      *err = "--eval-bins runs no simulation: it takes only --eval-bins-truth, --eval-bins-report, --eval-bins-bins, --eval-bins-contigs and --device ('" +
             first_not_bin + "' given)";
      return false;
    }
    if (a->eval_bins_truth.empty()) { *err = "--eval-bins needs --eval-bins-truth"; return false; }
    if (a->eval_bins_report.empty()) { *err = "--eval-bins needs --eval-bins-report"; return false; }
    return true;
  }
  if (!first_corr.empty()) {  // the eighth mode without a simulation
    if (a->eval_corrected.empty()) { *err = first_corr + " needs --eval-corrected"; return false; }
    if (!first_not_corr.empty()) {
      *err = "--eval-corrected runs no simulation: it takes only --eval-corrected-truth, --eval-corrected-report, --eval-corrected-reads, "
             "--eval-corrected-fasta and --device ('" + first_not_corr + "' given)";
      return false;
    }
    if (a->eval_corrected_truth.empty()) { *err = "--eval-corrected needs --eval-corrected-truth"; return false; }
    if (a->eval_corrected_report.empty()) { *err = "--eval-corrected needs --eval-corrected-report"; return false; }
    return true;
  }
  if (a->single_reads) { *err = "--single-reads needs --fit-from-sam"; return false; }
  if (a->sam_sorted && a->sam.empty()) { *err = "--sam-sorted needs --sam"; return false; }
  if (a->sam_sorted && !a->devices.empty()) { *err = "--sam-sorted does not combine with --devices: use --device"; return false; }
  if (a->bam_sorted && a->bam.empty()) { *err = "--bam-sorted needs --bam"; return false; }
  if (!a->bam_index.empty() && !a->bam_sorted) { *err = "--bam-index needs --bam-sorted"; return false; }
  if (!a->strain_sites.empty() && !a->with_ani) { *err = "--strain-sites needs --with-ani"; return false; }
  if (!a->strain_vcf.empty() && !a->with_ani) { *err = "--strain-vcf needs --with-ani"; return false; }
  // cli.rs:88-92: ArgGroup "genomes" is required, and --output has no default
  if (a->genome.empty() && !a->genome_file) { *err = "one of --genome / --genome-file is required"; return false; }
  if (!a->genome.empty() && a->genome_file) { *err = "--genome and --genome-file cannot be used together"; return false; }
  if (a->output.empty()) { *err = "--output is required"; return false; }
  return true;
}

std::unique_ptr<ErrorProfile> determine_error_profile(const CliArgs& args, std::string* err) {
  std::unique_ptr<ErrorProfile> out;
  switch (args.error_profile) {
    case ErrorProfileKind::PerfectShort: {  // cli.rs:231-234
      auto p = std::make_unique<PerfectShortErrorProfile>();
      p->read_length = args.read_length; p->insert_size = args.insert_size;
      return p;
    }
    case ErrorProfileKind::MinimalShort: {  // cli.rs:235-241: stds fixed at 75 / 15
      auto p = std::make_unique<MinimalShortErrorProfile>();
      p->read_length = args.read_length; p->insert_size = args.insert_size;
      p->mean_phred_score = args.mean_phred_score; p->insert_size_std = 75.0; p->read_length_std = 15.0;
      return p;
    }
    case ErrorProfileKind::PerfectLong:    // cli.rs:283
    case ErrorProfileKind::MinimalLong: {  // cli.rs:284-297
      const bool perfect = args.error_profile == ErrorProfileKind::PerfectLong;
      std::unique_ptr<MinimalLongErrorProfile> p = perfect ? std::make_unique<PerfectLongErrorProfile>() : std::make_unique<MinimalLongErrorProfile>();
      if (!perfect) p->mean_phred_score = args.mean_phred_score;
      if (!perfect) p->read_length = args.read_length < 400 ? 20000 : args.read_length;
      if (!perfect) p->read_length_std = args.read_length < 400 ? args.read_length_std : 5000.0;
      if (args.gamma) { p->gamma_mean = args.gamma->first; p->gamma_std = args.gamma->second; }
      out = std::move(p);
      break;
    }
    case ErrorProfileKind::CustomLong:    // extension: the same object, driven through simulate_long_reads
    case ErrorProfileKind::CustomShort: {  // cli.rs:255-272
      if (!args.custom_profile) { *err = "--custom-profile is required with --error-profile custom-short / custom-long"; return nullptr; }
      std::string e2;
      auto p = CustomShortErrorProfile::from_path(*args.custom_profile, &e2);
      if (!p) { *err = "Error parsing custom error profile: " + e2; return nullptr; }
      if (args.error_profile == ErrorProfileKind::CustomShort) return p;
      out = std::move(p);
      break;
    }
  }
  if (!out) { *err = "unknown error profile"; return nullptr; }
  // the long-read kinds: the extensions --per-read-lengths / --uniform-start
  if (args.per_read_lengths) out->length_mode = SIMMR_LEN_PER_READ;
  if (args.uniform_start) out->long_start_mode = SIMMR_START_UNIFORM;
  return out;
}

std::unique_ptr<AbundanceProfile> determine_abundance_profile(const CliArgs& args,
                                                              std::optional<std::vector<double>> abundances) {
  switch (args.abundance_profile) {  // cli.rs:306-320
    case AbundanceProfileKind::Exact: return std::make_unique<ExactAbundanceProfile>();
    case AbundanceProfileKind::Uniform: {
      auto p = std::make_unique<UniformAbundanceProfile>();
      p->size_adjusted = args.size_adjusted;
      return p;
    }
    case AbundanceProfileKind::Custom: {
      auto p = std::make_unique<CustomAbundanceProfile>();
      p->size_adjusted = args.size_adjusted;
      p->abundances = abundances.value_or(std::vector<double>());
      return p;
    }
  }
  return nullptr;
}

}  // namespace simmr_host

// ---- plain-C views for the CPU tests (ctypes): no GPU, no simulation ------------
extern "C" {
using namespace simmr_host;

// returns a malloc'ed string (caller frees with simmr_host_free)
static char* dup_str(const std::string& s) {
  char* p = (char*)malloc(s.size() + 1);
  memcpy(p, s.c_str(), s.size() + 1);
  return p;
}
void simmr_host_free(void* p) { free(p); }
// genomes that carry names only: genome_id[g] / n_contigs[g] per genome slot, sequence_id flattened genome by genome (the
// shape of simmr_fastq_names)
static std::vector<Genome> genomes_from_names(uint32_t n_genomes, const char* const* genome_id, const uint32_t* n_contigs,
                                              const char* const* sequence_id) {
  std::vector<Genome> genomes(n_genomes);
  size_t at = 0;
  for (uint32_t g = 0; g < n_genomes; g++) {
    genomes[g].uuid = genome_id[g];
    for (uint32_t c = 0; c < n_contigs[g]; c++) { Seq s; s.id = sequence_id[at++]; genomes[g].sequence.push_back(std::move(s)); }
  }
  return genomes;
}
// the PRODUCT's builder of the counter mode's splice tables (csrc/custom_model.hpp: what engine.hip uploads), for the CPU
// test that enumerates the law the tables encode (the test tree's custom-profile specification tests)
uint32_t simmr_host_ctr_splice_tables(const uint32_t* alt, const float* w, uint32_t n, uint32_t self_code, int has_self,
                                      uint32_t* thr, uint32_t* alias) {
  return simmr::ctr_splice_tables(alt, w, n, self_code, has_self != 0, thr, alias);
}
// The SAM header of sam_header_text for n names and lengths.  Returns the text, or "ERR\t..." .
char* simmr_host_sam_header(uint32_t n, const char* const* rname, const uint64_t* length) {
  std::string out, err;
  if (!sam_header_text(std::vector<std::string>(rname, rname + n), std::vector<uint64_t>(length, length + n), &out, &err)) return dup_str("ERR\t" + err);
  return dup_str(out);
}
// The header for a coordinate-sorted file
char* simmr_host_sam_header_sorted(uint32_t n, const char* const* rname, const uint64_t* length) {
  std::string out, err;
  if (!sam_header_text(std::vector<std::string>(rname, rname + n), std::vector<uint64_t>(length, length + n), &out, &err, true)) return dup_str("ERR\t" + err);
  return dup_str(out);
}
// sam_merge_sorted_runs over runs given as plain arrays: run k has run_lines[k] lines, its keys and lengths follow those of
// run k - 1 in key[] / len[], its text begins at run_offset[k] of src (src_bytes bytes).  The merged bytes go to dst
// (dst_capacity bytes); returns their number, or -1 if a run leaves src, the output leaves dst, or the merge fails.
int64_t simmr_host_sam_merge(uint32_t n_runs, const uint64_t* run_lines, const uint64_t* run_offset, const uint64_t* key, const uint64_t* len,
                             const char* src, uint64_t src_bytes, char* dst, uint64_t dst_capacity) {
  std::vector<SamSortedRun> runs(n_runs);
  size_t at = 0;
  for (uint32_t k = 0; k < n_runs; k++) {
    runs[k].key.assign(key + at, key + at + run_lines[k]);
    runs[k].len.assign(len + at, len + at + run_lines[k]);
    runs[k].offset = run_offset[k];
    at += run_lines[k];
  }
  uint64_t written = 0;
  const bool ok = sam_merge_sorted_runs(
      runs,
      [&](uint64_t off, size_t n, char* p) { if (off > src_bytes || n > src_bytes - off) return false; memcpy(p, src + off, n); return true; },
      [&](const char* p, size_t n) { if (n > dst_capacity - written) return false; memcpy(dst + written, p, n); written += n; return true; });
  return ok ? (int64_t)written : -1;
}
// RNAME of a sequence id (sam_rname)
char* simmr_host_sam_rname(const char* sequence_id) { return dup_str(sam_rname(sequence_id)); }
char* simmr_host_normalize(const char* raw, uint64_t n) { return dup_str(normalize(std::string(raw, n))); }
char* simmr_host_format_f64(double v) { return dup_str(format_f64_display(v)); }
char* simmr_host_format_header(const char* fmt, const char* genome_id, uint32_t read_id, const char* seq_id,
                               uint64_t start, uint64_t end, int revcomp, int pair) {
  return dup_str(format_header(fmt, genome_id, read_id, seq_id, start, end, revcomp != 0, pair));
}
// Loads a FASTA; writes a description "n_seqs\tsize\n" + per sequence "id\tsize\tlen\tseq\n"
char* simmr_host_load_fasta(const char* path, int contiguous) {
  Genome g;
  std::string err;
  if (!Genome::from_fasta(path, contiguous != 0, &g, &err)) return dup_str("ERR\t" + err);
  std::string out = std::to_string(g.num_seqs) + "\t" + std::to_string(g.size) + "\n";
  for (const Seq& s : g.sequence)
    out += s.id + "\t" + std::to_string(s.size) + "\t" + std::to_string(s.seq.size()) + "\t" + s.seq + "\n";
  return dup_str(out);
}
// The truth TSV of write_truth_tsv for columns given as plain arrays, names as for genomes_from_names.  Returns "OK", or "ERR\t..." .
char* simmr_host_truth_tsv(uint64_t n_reads, int paired, const uint32_t* read_id, const uint32_t* genome, const uint32_t* contig,
                           const uint64_t* start, const uint64_t* end, const uint8_t* flags, const uint32_t* nm,
                           const uint64_t* edit_off, const uint32_t* edit_pos, const uint8_t* edit_ref, const uint8_t* edit_alt,
                           const uint8_t* edit_qual, uint32_t qual_offset, uint32_t n_genomes, const char* const* genome_id,
                           const uint32_t* n_contigs, const char* const* sequence_id, int with_header, const char* path) {
  const std::vector<Genome> genomes = genomes_from_names(n_genomes, genome_id, n_contigs, sequence_id);
  HostReads h;
  h.n_reads = n_reads; h.paired = paired != 0;
  h.read_id.assign(read_id, read_id + n_reads); h.genome.assign(genome, genome + n_reads); h.contig.assign(contig, contig + n_reads);
  h.start.assign(start, start + n_reads); h.end.assign(end, end + n_reads); h.flags.assign(flags, flags + n_reads);
  HostTruth t;
  const uint64_t m = n_reads ? edit_off[n_reads] : 0;
  t.nm.assign(nm, nm + n_reads); t.edit_off.assign(edit_off, edit_off + n_reads + 1);
  t.edit_pos.assign(edit_pos, edit_pos + m); t.edit_ref.assign(edit_ref, edit_ref + m);
  t.edit_alt.assign(edit_alt, edit_alt + m); t.edit_qual.assign(edit_qual, edit_qual + m);
  std::string err;
  if (!write_truth_tsv(genomes, h, t, qual_offset, path, with_header != 0, &err)) return dup_str("ERR\t" + err);
  return dup_str("OK");
}
// The strain-site TSV of write_strain_sites_tsv for columns given as plain arrays; the genome's names: its id and its
// n_contigs sequence ids.  Returns "OK", or "ERR\t..." .
char* simmr_host_strain_tsv(uint64_t n_sites, const uint32_t* contig, const uint64_t* pos, const uint8_t* ref, const uint8_t* alt,
                            const char* genome_id, uint32_t n_contigs, const char* const* sequence_id, int with_header, const char* path) {
  const std::vector<Genome> genomes = genomes_from_names(1, &genome_id, &n_contigs, sequence_id);
  HostStrainSites s;
  s.contig.assign(contig, contig + n_sites); s.pos.assign(pos, pos + n_sites);
  s.ref.assign(ref, ref + n_sites); s.alt.assign(alt, alt + n_sites);
  std::string err;
  if (!write_strain_sites_tsv(genomes[0], s, path, with_header != 0, &err)) return dup_str("ERR\t" + err);
  return dup_str("OK");
}
// The VCF of write_strain_vcf for site columns and a count table given as plain arrays (counts: n_sites * 10 entries); names in
// the shape of simmr_host_truth_tsv, contig_len flattened like sequence_id.  Returns "OK", or "ERR\t..." .
char* simmr_host_strain_vcf(uint64_t n_sites, const uint32_t* genome, const uint32_t* contig, const uint64_t* pos, const uint8_t* ref,
                            const uint8_t* alt, const uint32_t* counts, uint32_t n_genomes, const char* const* genome_id,
                            const uint32_t* n_contigs, const char* const* sequence_id, const uint64_t* contig_len, const char* path) {
  const std::vector<Genome> genomes = genomes_from_names(n_genomes, genome_id, n_contigs, sequence_id);
  std::vector<std::vector<uint64_t>> lens(n_genomes);
  for (uint32_t g = 0, at = 0; g < n_genomes; at += n_contigs[g], g++) lens[g].assign(contig_len + at, contig_len + at + n_contigs[g]);
  HostStrainSites s;
  s.contig.assign(contig, contig + n_sites); s.pos.assign(pos, pos + n_sites);
  s.ref.assign(ref, ref + n_sites); s.alt.assign(alt, alt + n_sites);
  std::string err;
  if (!write_strain_vcf(genomes, lens, s, std::vector<uint32_t>(genome, genome + n_sites), std::vector<uint32_t>(counts, counts + n_sites * 10), path, &err))
    return dup_str("ERR\t" + err);
  return dup_str("OK");
}
// The model file of write_fit_model for an info and columns in host memory.  Returns "OK", or "ERR\t..." .
char* simmr_host_fit_model(const simmr_fit_info* info, const simmr_fit_out* cols, const char* path) {
  std::string err;
  if (!info || !cols || !path) return dup_str("ERR\tNULL argument");
  if (!write_fit_model(*info, *cols, path, &err)) return dup_str("ERR\t" + err);
  return dup_str("OK");
}
// The statistics TSV of write_stats_tsv for a simmr_run_stats in host memory.  Returns "OK", or "ERR\t..." .
char* simmr_host_stats_tsv(const simmr_run_stats* st, const char* path) {
  std::string err;
  if (!st || !path) return dup_str("ERR\tNULL argument");
  if (!write_stats_tsv(*st, path, &err)) return dup_str("ERR\t" + err);
  return dup_str("OK");
}
// The two depth TSVs of write_depth_tsv / write_depth_track_tsv for rows and window columns in host memory; names in the
// shape of simmr_host_truth_tsv.  track_path may be NULL (then window and win_* are not read).  Returns "OK", or "ERR\t..." .
char* simmr_host_depth_tsv(const simmr_depth_contig* rows, uint64_t n_rows, uint32_t n_genomes, const char* const* genome_id,
                           const uint32_t* n_contigs, const char* const* sequence_id, const char* path, uint32_t window,
                           const uint64_t* win_sum, const uint32_t* win_covered, const uint32_t* win_max, const char* track_path) {
  const std::vector<Genome> genomes = genomes_from_names(n_genomes, genome_id, n_contigs, sequence_id);
  std::string err;
  if (path && !write_depth_tsv(genomes, rows, n_rows, path, &err)) return dup_str("ERR\t" + err);
  if (track_path && !write_depth_track_tsv(genomes, rows, n_rows, window, win_sum, win_covered, win_max, track_path, &err)) return dup_str("ERR\t" + err);
  return dup_str("OK");
}
// The gold-assembly FASTA and TSV of write_gold_fasta / write_gold_regions_tsv for columns in host memory (seq_off: n_regions + 1
// entries; seq: seq_off[n_regions] bytes); names in the shape of simmr_host_truth_tsv.  Either path may be NULL.  Returns
// "OK", or "ERR\t..." .
char* simmr_host_gold_files(uint64_t n_regions, const uint32_t* genome, const uint32_t* contig, const uint64_t* start, const uint64_t* len,
                            const uint64_t* depth_sum, const uint64_t* seq_off, const uint8_t* seq, uint32_t n_genomes,
                            const char* const* genome_id, const uint32_t* n_contigs, const char* const* sequence_id, const char* fasta_path,
                            const char* tsv_path) {
  const std::vector<Genome> genomes = genomes_from_names(n_genomes, genome_id, n_contigs, sequence_id);
  HostRegions r;
  r.genome.assign(genome, genome + n_regions); r.contig.assign(contig, contig + n_regions); r.start.assign(start, start + n_regions);
  r.len.assign(len, len + n_regions); r.depth_sum.assign(depth_sum, depth_sum + n_regions); r.seq_off.assign(seq_off, seq_off + n_regions + 1);
  if (seq) r.seq.assign(seq, seq + seq_off[n_regions]);
  std::string err;
  if (fasta_path && !write_gold_fasta(genomes, r, fasta_path, &err)) return dup_str("ERR\t" + err);
  if (tsv_path && !write_gold_regions_tsv(genomes, r, tsv_path, &err)) return dup_str("ERR\t" + err);
  return dup_str("OK");
}
char* simmr_host_parse_genome_file(const char* path) {
  std::vector<GenomeRecord> recs;
  std::string err;
  if (!parse_genome_file(path, &recs, &err)) return dup_str("ERR\t" + err);
  std::string out;
  for (const auto& r : recs)
    out += r.filepath + "\t" + (r.uuid ? *r.uuid : std::string("<none>")) + "\t" +
           (r.abundance ? format_f64_display(*r.abundance) : std::string("<none>")) + "\n";
  return dup_str(out);
}
}
