// main.cpp — `simmr-hip`: the reference's run_main (simmr/src/main.rs:20-268)
// over the C ABI of libsimmr_hip.so.  Same flags, same output files:
// interleaved FASTQ (fastq.rs) and "<output>.tsv" metadata (files.rs:100-134).
#include <cstring>
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <sys/stat.h>

#include <algorithm>
#include <condition_variable>
#include <fstream>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

#include "cli_common.hpp"
#include "eval_cli.hpp"
#include "simmr_host.hpp"

using namespace simmr_host;

static void reads_not_written(const std::string& err) { fprintf(stderr, "ERROR simmr-hip: Failed to write reads to the output file: %s\n", err.c_str()); }
static bool exists(const std::string& p) { struct stat st; return stat(p.c_str(), &st) == 0; }
static bool is_regular_file(const std::string& p) { struct stat st; return stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode); }

// Device allocations that are freed together, and the copy of a device array into a host vector.
struct DeviceMem {
  std::vector<void*> allocs;
  ~DeviceMem() { for (void* p : allocs) (void)hipFree(p); }
  template <class T> bool alloc(T** dst, size_t n) {
    void* p = nullptr;
    if (hipMalloc(&p, (n ? n : 1) * sizeof(T)) != hipSuccess) return false;
    allocs.push_back(p);
    *dst = (T*)p;
    return true;
  }
  template <class T> static bool fetch(std::vector<T>* h, const T* dev, size_t n) {
    h->resize(n);
    return n == 0 || hipMemcpy(h->data(), dev, n * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess;
  }
};

struct DeviceOut {
  simmr_reads_out o{};
  DeviceMem mem;
  bool init(uint64_t n_reads, uint64_t total_bases, uint32_t slot_bytes) {
    o.slot_bytes = slot_bytes;  // simmr_plan_info.slot_bytes: the layout the plan in force emits
    o.seq_capacity = total_bases + 32;
    o.reads_capacity = n_reads;
    o.qual_offset = 33;  // util::encode_quality_scores (util.rs:46-57)
    return mem.alloc(&o.seq, o.seq_capacity) && mem.alloc(&o.qual, o.seq_capacity) && mem.alloc(&o.seq_off, n_reads + 1) &&
           mem.alloc(&o.start, n_reads) && mem.alloc(&o.end, n_reads) && mem.alloc(&o.contig, n_reads) &&
           mem.alloc(&o.genome, n_reads) && mem.alloc(&o.read_id, n_reads) && mem.alloc(&o.flags, n_reads);
  }
  bool to_host(uint64_t n_reads, uint64_t total_bases, bool paired, HostReads* h) {
    h->n_reads = n_reads; h->paired = paired;
    if (!(mem.fetch(&h->seq, o.seq, total_bases) && mem.fetch(&h->qual, o.qual, total_bases) && mem.fetch(&h->seq_off, o.seq_off, n_reads + 1) &&
          mem.fetch(&h->start, o.start, n_reads) && mem.fetch(&h->end, o.end, n_reads) && mem.fetch(&h->contig, o.contig, n_reads) &&
          mem.fetch(&h->genome, o.genome, n_reads) && mem.fetch(&h->read_id, o.read_id, n_reads) && mem.fetch(&h->flags, o.flags, n_reads)))
      return false;
    if (o.slot_bytes == SIMMR_SLOT16) {
      // the consumer's side of the slot layout (include/simmr_hip.h): L = |end - start|, bases from seq_off[r], qualities
      // from seq_off[r] & ~15 — closed up in place into the compact form write_to_fastq reads (reads ascend in both)
      uint64_t at = 0;
      for (uint64_t r = 0; r < n_reads; r++) {
        const uint64_t L = h->end[r] > h->start[r] ? h->end[r] - h->start[r] : h->start[r] - h->end[r];
        const uint64_t sb = h->seq_off[r], qb = sb & ~15ull;
        memmove(h->seq.data() + at, h->seq.data() + sb, L);
        memmove(h->qual.data() + at, h->qual.data() + qb, L);
        h->seq_off[r] = at;
        at += L;
      }
      h->seq_off[n_reads] = at;
      h->seq.resize(at); h->qual.resize(at);
    }
    return true;
  }
};

// The truth columns of one range's reads (simmr_truth_plan / simmr_truth_emit on the columns `d`): on the device in `o`, owned
// by `mem`, and copied to the host if `t` is given.
static bool device_truth(simmr_engine* eng, const simmr_reads_out* reads, uint64_t n_reads, DeviceMem* mem, simmr_truth_out* o, HostTruth* t,
                         std::string* err) {
  uint64_t m = 0;
  if (simmr_truth_plan(eng, reads, n_reads, &m) != SIMMR_OK) { *err = simmr_last_error(eng); return false; }
  *o = simmr_truth_out{};
  o->reads_capacity = n_reads; o->edits_capacity = m;
  if (!(mem->alloc(&o->nm, n_reads) && mem->alloc(&o->edit_off, n_reads + 1) && mem->alloc(&o->edit_pos, m) && mem->alloc(&o->edit_ref, m) &&
        mem->alloc(&o->edit_alt, m) && mem->alloc(&o->edit_qual, m))) { *err = "device allocation failed"; return false; }
  if (simmr_truth_emit(eng, reads, o) != SIMMR_OK) { *err = simmr_last_error(eng); return false; }
  if (t && !(mem->fetch(&t->nm, o->nm, n_reads) && mem->fetch(&t->edit_off, o->edit_off, n_reads + 1) && mem->fetch(&t->edit_pos, o->edit_pos, m) &&
             mem->fetch(&t->edit_ref, o->edit_ref, m) && mem->fetch(&t->edit_alt, o->edit_alt, m) && mem->fetch(&t->edit_qual, o->edit_qual, m))) { *err = "copy back failed"; return false; }
  return true;
}

// `--sam` / `--bam`, before any device work: every sequence of the run's FASTA files gets its RNAME (the first word of its id; under
// --contiguous a genome is the one sequence "whole genome"), which has to be a SAM reference name that no other sequence of the
// run has.  false with the one message that names the sequence.  A file that cannot be read is left to the loading code.
static bool sam_check_names(const CliArgs& args, std::string* err) {
  const std::string flag = args.sam.empty() ? "--bam: " : "--sam: ";
  std::vector<std::string> paths = args.genome;
  if (args.genome_file) {
    std::vector<GenomeRecord> records;
    std::string e;
    if (!parse_genome_file(*args.genome_file, &records, &e)) return true;
    for (const GenomeRecord& r : records) paths.push_back(r.filepath);
  }
  std::vector<std::pair<std::string, std::string>> seen;  // RNAME, "sequence 'id' of path"
  for (const std::string& path : paths) {
    FastaRecords recs;
    std::string e;
    if (!scan_fasta(path, &recs, &e)) continue;
    std::vector<std::string> ids = args.contiguous ? std::vector<std::string>{"whole genome"} : recs.ids;
    for (const std::string& id : ids) {
      const std::string rname = sam_rname(id), who = "sequence '" + id + "' of " + path;
      if (!sam_rname_legal(rname)) { *err = flag + who + " gets the RNAME '" + rname + "', which is not a SAM reference name"; return false; }
      for (const auto& s : seen)
        if (s.first == rname) { *err = flag + who + " gets the RNAME '" + rname + "', which " + s.second + " has already"; return false; }
      seen.emplace_back(rname, who);
    }
    if (args.bam_sorted) {  // a BAI index reaches 2^29 bases: no sequence body may hold that many (line ends aside)
      uint64_t whole = 0;
      for (size_t k = 0; k < recs.body.size(); k++) {
        uint64_t bases = 0;
        for (size_t i = recs.body[k].first; i < recs.body[k].first + recs.body[k].second && i < recs.data.size(); i++)
          bases += recs.data[i] != '\n' && recs.data[i] != '\r';
        whole += bases;
        if ((args.contiguous ? whole : bases) >= (1ull << 29)) {
          *err = "--bam-sorted: " + (args.contiguous ? std::string("the genome") : "sequence '" + recs.ids[k] + "'") + " of " + path +
                 " has 2^29 bases or more: a BAI index does not reach there (CSI is not written)";
          return false;
        }
      }
    }
  }
  return true;
}

// `--depth` / `--depth-track`: depth[] of every range added so far (simmr_depth_emit), its contig rows and windows
// (simmr_depth_summarize), and the two files.
static bool write_depth_files(simmr_engine* eng, const CliArgs& args, const std::vector<Genome>& genomes, uint64_t n_positions,
                              uint64_t n_contigs, std::string* err) {
  DeviceMem mem;
  uint32_t* depth = nullptr;
  if (!mem.alloc(&depth, n_positions)) { *err = "device allocation failed"; return false; }
  if (simmr_depth_emit(eng, depth, n_positions) != SIMMR_OK) { *err = simmr_last_error(eng); return false; }
  std::vector<simmr_depth_contig> rows(std::max<uint64_t>(n_contigs, 1));
  const bool track = !args.depth_track.empty();
  simmr_depth_windows win{};
  if (track) {  // a call without room answers SIMMR_ERANGE and says how many windows the staged lengths make
    const int rc = simmr_depth_summarize(eng, depth, args.depth_window, nullptr, 0, nullptr, &win);
    if (rc != SIMMR_OK && rc != SIMMR_ERANGE) { *err = simmr_last_error(eng); return false; }
    win.capacity = win.n_windows;
    if (!(mem.alloc(&win.sum, win.capacity) && mem.alloc(&win.covered, win.capacity) && mem.alloc(&win.max, win.capacity))) { *err = "device allocation failed"; return false; }
  }
  if (simmr_depth_summarize(eng, depth, track ? args.depth_window : 0u, rows.data(), rows.size(), nullptr, track ? &win : nullptr) != SIMMR_OK) { *err = simmr_last_error(eng); return false; }
  if (!args.depth.empty() && !write_depth_tsv(genomes, rows.data(), n_contigs, args.depth, err)) return false;
  if (!track) return true;
  std::vector<uint64_t> ws;
  std::vector<uint32_t> wc, wm;
  if (!(mem.fetch(&ws, win.sum, win.n_windows) && mem.fetch(&wc, win.covered, win.n_windows) && mem.fetch(&wm, win.max, win.n_windows))) { *err = "copy back failed"; return false; }
  return write_depth_track_tsv(genomes, rows.data(), n_contigs, args.depth_window, ws.data(), wc.data(), wm.data(), args.depth_track, err);
}

// `--gold-assembly` / `--gold-regions`: the regions of the run's depth[] (simmr_regions_plan / simmr_regions_emit over what
// simmr_depth_emit gives of every range added so far), copied to the host and written as FASTA and as a TSV.
static bool write_gold_files(simmr_engine* eng, const CliArgs& args, const std::vector<Genome>& genomes, uint64_t n_positions, std::string* err) {
  DeviceMem mem;
  uint32_t* depth = nullptr;
  if (!mem.alloc(&depth, n_positions)) { *err = "device allocation failed"; return false; }
  if (simmr_depth_emit(eng, depth, n_positions) != SIMMR_OK) { *err = simmr_last_error(eng); return false; }
  uint64_t n = 0, nb = 0;
  if (simmr_regions_plan(eng, depth, args.gold_min_depth, args.gold_min_length, &n, &nb) != SIMMR_OK) { *err = simmr_last_error(eng); return false; }
  const bool fasta = !args.gold_assembly.empty();
  simmr_regions_out o{};
  o.capacity = n;
  o.seq_capacity = fasta ? nb + 16 : 0;
  if (!(mem.alloc(&o.genome, n) && mem.alloc(&o.contig, n) && mem.alloc(&o.start, n) && mem.alloc(&o.len, n) && mem.alloc(&o.depth_sum, n) &&
        mem.alloc(&o.seq_off, n + 1) && (!fasta || mem.alloc(&o.seq, o.seq_capacity)))) { *err = "device allocation failed"; return false; }
  if (simmr_regions_emit(eng, depth, &o) != SIMMR_OK) { *err = simmr_last_error(eng); return false; }
  HostRegions h;
  if (!(mem.fetch(&h.genome, o.genome, n) && mem.fetch(&h.contig, o.contig, n) && mem.fetch(&h.start, o.start, n) && mem.fetch(&h.len, o.len, n) &&
        mem.fetch(&h.depth_sum, o.depth_sum, n) && mem.fetch(&h.seq_off, o.seq_off, n + 1) && (!fasta || mem.fetch(&h.seq, o.seq, nb)))) { *err = "copy back failed"; return false; }
  if (fasta && !write_gold_fasta(genomes, h, args.gold_assembly, err)) return false;
  return args.gold_regions.empty() || write_gold_regions_tsv(genomes, h, args.gold_regions, err);
}

// `--with-ani` / `--strain-sites`: genome i of the run becomes a strain on every engine (simmr_strain_plan /
// simmr_strain_apply with the seed run seed + 0x9E3779B97F4A7C15 (i + 1)); the outcome is a function of the inputs, so the
// engines' copies agree, and the sites are listed from the first engine.  `--strain-vcf`: the sites of every genome are kept
// in `keep`, back to back in genome order, with the genome's index in `keep_genome`.
static bool diverge_genomes(const std::vector<simmr_engine*>& engs, const CliArgs& args, const std::vector<Genome>& genomes,
                            uint64_t run_seed, HostStrainSites* keep, std::vector<uint32_t>* keep_genome, std::string* err) {
  const bool list = !args.strain_sites.empty(), kept = !args.strain_vcf.empty();
  if (list && is_regular_file(args.strain_sites)) remove(args.strain_sites.c_str());
  for (size_t gi = 0; gi < genomes.size(); gi++) {
    const uint64_t seed = run_seed + 0x9E3779B97F4A7C15ull * (uint64_t)(gi + 1);
    for (size_t k = 0; k < engs.size(); k++) {
      uint64_t n = 0;
      if (simmr_strain_plan(engs[k], (uint32_t)gi, *args.with_ani / 100.0, seed, &n) != SIMMR_OK) { *err = simmr_last_error(engs[k]); return false; }
      if (k > 0 || !(list || kept)) {
        if (simmr_strain_apply(engs[k], (uint32_t)gi, nullptr) != SIMMR_OK) { *err = simmr_last_error(engs[k]); return false; }
        continue;
      }
      DeviceMem mem;  // (on the first engine's device: the plan call selected it)
      simmr_strain_out o{};
      o.capacity = n;
      if (!(mem.alloc(&o.contig, n) && mem.alloc(&o.pos, n) && mem.alloc(&o.ref, n) && mem.alloc(&o.alt, n))) { *err = "device allocation failed"; return false; }
      if (simmr_strain_apply(engs[k], (uint32_t)gi, &o) != SIMMR_OK) { *err = simmr_last_error(engs[k]); return false; }
      HostStrainSites h;
      if (!(mem.fetch(&h.contig, o.contig, n) && mem.fetch(&h.pos, o.pos, n) && mem.fetch(&h.ref, o.ref, n) && mem.fetch(&h.alt, o.alt, n))) { *err = "copy back failed"; return false; }
      if (list && !write_strain_sites_tsv(genomes[gi], h, args.strain_sites, gi == 0, err)) return false;
      if (kept) {
        keep->contig.insert(keep->contig.end(), h.contig.begin(), h.contig.end());
        keep->pos.insert(keep->pos.end(), h.pos.begin(), h.pos.end());
        keep->ref.insert(keep->ref.end(), h.ref.begin(), h.ref.end());
        keep->alt.insert(keep->alt.end(), h.alt.begin(), h.alt.end());
        keep_genome->insert(keep_genome->end(), h.pos.size(), (uint32_t)gi);
      }
    }
  }
  return true;
}

// `--strain-vcf`: the table of every range added so far (simmr_pileup_read), the sequences' lengths from the layout of depth[]
// (the engine's own contig table: exact under --contiguous too), and the file.
static bool write_vcf_file(simmr_engine* eng, const CliArgs& args, const std::vector<Genome>& genomes, const HostStrainSites& sites,
                           const std::vector<uint32_t>& site_genome, uint64_t n_positions, std::string* err) {
  std::vector<std::vector<uint64_t>> lens(genomes.size());
  std::vector<uint64_t> firsts;
  for (size_t g = 0; g < genomes.size(); g++)
    for (size_t c = 0; c < genomes[g].sequence.size(); c++) {
      uint64_t first = 0;
      if (simmr_depth_contig_first(eng, (uint32_t)g, (uint32_t)c, &first) != SIMMR_OK) { *err = simmr_last_error(eng); return false; }
      firsts.push_back(first);
    }
  firsts.push_back(n_positions);
  for (size_t g = 0, k = 0; g < genomes.size(); g++)
    for (size_t c = 0; c < genomes[g].sequence.size(); c++, k++) lens[g].push_back(firsts[k + 1] - firsts[k]);
  const uint64_t n = sites.pos.size();
  DeviceMem mem;
  uint32_t* table = nullptr;
  std::vector<uint32_t> counts;
  if (!mem.alloc(&table, n * 10)) { *err = "device allocation failed"; return false; }
  if (simmr_pileup_read(eng, table, n) != SIMMR_OK) { *err = simmr_last_error(eng); return false; }
  if (!mem.fetch(&counts, table, n * 10)) { *err = "copy back failed"; return false; }
  return write_strain_vcf(genomes, lens, sites, site_genome, counts, args.strain_vcf, err);
}

// the text buffer of the drains: what one copy to the host moves, and what a window of --overlaps holds
static constexpr size_t TEXT_CHUNK = 256u << 20;

// The side outputs of a run: --truth, --sam, --bam, --overlaps, --stats, --fit-model, --depth, --depth-track, --gold-assembly, --gold-regions and --strain-vcf.  They read the columns, so a run that wants one
// takes the column route (the same bytes, include/simmr_hip.h).  A call that answers false leaves its message in `err`.
struct SideOutputs {
  explicit SideOutputs(const CliArgs& args) : a(args) {}
  const CliArgs& a;
  std::string err;
  HostTruth truth;           // of the range last added, until write_range has written it
  uint32_t qual_offset = 33;
  uint64_t depth_positions = 0, depth_contigs = 0;
  HostStrainSites sites;             // --strain-vcf: what diverge_genomes kept, and each site's genome
  std::vector<uint32_t> site_genome;
  std::vector<std::string> sam_names;  // --sam: RNAME per sequence, genome by genome (simmr_sam_names), and where each genome's begin
  std::vector<uint32_t> sam_genome, sam_contigs;
  std::vector<const char*> sam_name_ptrs;  // what `sn` points into: built once, by begin_sam
  simmr_sam_names sn{};
  // --sam-sorted: every range's lines come sorted from the device, a run with the key and the length of each line (16 bytes a
  // read); finish() merges the runs (SortedRunSpill, simmr_host.hpp: one run in memory, several in a temporary file beside the SAM file).
  SortedRunSpill sam_spill{a.sam};
  // --bam-sorted: the same shape for the records of every range, with the ends of the records beside the keys; the header waits
  // for finish(), which frames header and records as one stream.  The state object of simmr_bam_sort_* belongs to the owner of
  // the engines (it has to go before its engine).
  SortedRunSpill bam_spill{a.bam};
  std::vector<std::vector<uint32_t>> bam_ends;
  std::vector<uint64_t> bam_lengths;
  std::string bam_head;
  simmr_bam_sort** bam_sort = nullptr;
  static constexpr size_t BAM_PIECE_BLOCKS = 1024;  // blocks of 65 280 source bytes a framing call takes
  bool run_paired = false;  // --overlaps: the run's reads are interleaved mates (set before begin)
  std::string bam_index_path() const { return a.bam_index.empty() ? a.bam + ".bai" : a.bam_index; }
  bool overlaps() const { return !a.overlaps.empty(); }
  bool vcf() const { return !a.strain_vcf.empty(); }
  bool sam() const { return !a.sam.empty(); }
  bool bam() const { return !a.bam.empty(); }
  bool depth_files() const { return !a.depth.empty() || !a.depth_track.empty(); }
  bool gold() const { return !a.gold_assembly.empty() || !a.gold_regions.empty(); }
  bool depth() const { return depth_files() || gold(); }  // (the gold-standard assembly is read off the run's depth[])
  bool fit() const { return !a.fit_model.empty(); }
  bool wanted() const { return !a.truth.empty() || sam() || bam() || overlaps() || !a.stats.empty() || fit() || depth() || vcf(); }
  bool fail(const char* flag, const std::string& what) { err = std::string(flag) + ": " + what; return false; }
  // true, with the message, if one of them is asked for together with --devices
  bool refuse_devices() {
    const char* flag = !a.truth.empty() ? "--truth" : !a.stats.empty() ? "--stats" : fit() ? "--fit-model" : depth_files() ? "--depth" : !a.gold_assembly.empty() ? "--gold-assembly" : gold() ? "--gold-regions" : vcf() ? "--strain-vcf" : sam() ? "--sam" : bam() ? "--bam" : overlaps() ? "--overlaps" : nullptr;
    if (flag && !a.devices.empty()) err = std::string(flag) + " does not combine with --devices: use --device";
    return flag && !a.devices.empty();
  }
  // the old files go, the truth file gets its header line (every range appends its reads), the tables start at zero
  // (the genomes are staged: depth[] covers all of them)
  bool begin(simmr_engine* eng, const std::vector<Genome>& genomes) {
    for (const std::string* f : {&a.truth, &a.sam, &a.bam, &a.overlaps, &a.stats, &a.fit_model, &a.depth, &a.depth_track, &a.gold_assembly, &a.gold_regions, &a.strain_vcf})
      if (!f->empty() && is_regular_file(*f)) remove(f->c_str());
    if (a.bam_sorted && is_regular_file(bam_index_path())) remove(bam_index_path().c_str());
    std::string e;
    if (overlaps() && simmr_overlap_reset(eng, run_paired ? 1 : 0) != SIMMR_OK) return fail("--overlaps", simmr_last_error(eng));
    if (!a.truth.empty() && !write_truth_tsv(genomes, HostReads{}, HostTruth{}, 33, a.truth, true, &e)) return fail("--truth", e);
    if ((sam() || bam()) && !begin_sam(eng, genomes)) return false;
    if (!a.stats.empty() && simmr_stats_reset(eng) != SIMMR_OK) return fail("--stats", simmr_last_error(eng));
    if (fit() && simmr_fit_reset(eng, a.fit_k, a.fit_max_alt, FIT_PAIR_CAPACITY) != SIMMR_OK) return fail("--fit-model", simmr_last_error(eng));
    // (--strain-vcf takes the sequences' lengths from the layout the depth reset records)
    if ((depth() || vcf()) && simmr_depth_reset(eng, &depth_positions, &depth_contigs) != SIMMR_OK) return fail("--depth", simmr_last_error(eng));
    return !vcf() || begin_pileup(eng);
  }
  // the names of the run's sequences as the device wants them, and the header: once, before the first range
  bool begin_sam(simmr_engine* eng, const std::vector<Genome>& genomes) {
    std::vector<uint64_t> lengths;
    for (size_t g = 0; g < genomes.size(); g++) {
      sam_genome.push_back((uint32_t)g);
      sam_contigs.push_back((uint32_t)genomes[g].sequence.size());
      for (const Seq& q : genomes[g].sequence) { sam_names.push_back(sam_rname(q.id)); lengths.push_back(q.size); }
    }
    for (const std::string& n : sam_names) sam_name_ptrs.push_back(n.c_str());
    sn = simmr_sam_names{(uint32_t)sam_genome.size(), sam_genome.data(), sam_contigs.data(), sam_name_ptrs.data()};
    std::string text, e;
    if (bam() && !begin_bam(eng, lengths)) return false;
    if (!sam()) return true;
    if (!sam_header_text(sam_names, lengths, &text, &e, a.sam_sorted)) return fail("--sam", e);
    OutFile f(a.sam, false);
    f.append(text);
    return f.close(&e) || fail("--sam", e);
  }
  // --bam: the file's head — magic, the header text of --sam (read order), the references — built here, framed on the device
  bool begin_bam(simmr_engine* eng, const std::vector<uint64_t>& lengths) {
    std::string text, e, head;
    if (!sam_header_text(sam_names, lengths, &text, &e, a.bam_sorted)) return fail("--bam", e);
    auto put32 = [&](uint32_t v) { for (int k = 0; k < 4; k++) head.push_back((char)(v >> (8 * k))); };
    head += "BAM\1";
    put32((uint32_t)text.size());
    head += text;
    put32((uint32_t)sam_names.size());
    for (size_t k = 0; k < sam_names.size(); k++) {
      if (lengths[k] >= (1ull << 31)) return fail("--bam", "sequence '" + sam_names[k] + "' has 2^31 bases or more: BAM's l_ref is an int32");
      put32((uint32_t)sam_names[k].size() + 1u);
      head.append(sam_names[k].c_str(), sam_names[k].size() + 1);
      put32((uint32_t)lengths[k]);
    }
    if (a.bam_sorted) {  // the header is framed with the records, as one stream, by finish_bam_sorted
      for (size_t k = 0; k < lengths.size(); k++)
        if (lengths[k] >= (1ull << 29)) return fail("--bam-sorted", "sequence '" + sam_names[k] + "' has 2^29 bases or more: a BAI index does not reach there");
      bam_head = head;
      bam_lengths = lengths;
      return true;
    }
    DeviceMem mem;
    uint8_t* src = nullptr;
    if (!mem.alloc(&src, head.size()) || hipMemcpy(src, head.data(), head.size(), hipMemcpyHostToDevice) != hipSuccess) return fail("--bam", "copy to the device failed");
    OutFile f(a.bam, false);
    return bam_append_framed(eng, &mem, src, head.size(), &f) && (f.close(&e) || fail("--bam", e));
  }
  // n bytes of device memory as BGZF blocks (simmr_bgzf_frame), fetched and appended to the file
  bool bam_append_framed(simmr_engine* eng, DeviceMem* mem, const uint8_t* src, uint64_t n, OutFile* f) {
    const uint64_t bound = simmr_bgzf_bound(n);
    uint8_t* blocks = nullptr;
    uint64_t written = 0;
    std::vector<uint8_t> h;
    if (!mem->alloc(&blocks, bound)) return fail("--bam", "device allocation failed");
    if (simmr_bgzf_frame(eng, src, n, blocks, bound, &written) != SIMMR_OK) return fail("--bam", simmr_last_error(eng));
    if (!mem->fetch(&h, (const uint8_t*)blocks, written)) return fail("--bam", "copy back failed");
    f->append(h.data(), h.size());
    return true;
  }
  // the records of one range: plan, emit, frame, fetch, append
  bool bam_range(simmr_engine* eng, const simmr_reads_out& reads, const simmr_truth_out& t, uint64_t n_reads, bool paired) {
    uint64_t total = 0;
    if (simmr_bam_plan(eng, &sn, &reads, &t, n_reads, paired ? 1 : 0, &total) != SIMMR_OK) return fail("--bam", simmr_last_error(eng));
    DeviceMem mem;
    uint8_t* rec = nullptr;
    if (!mem.alloc(&rec, total)) return fail("--bam", "device allocation failed");
    if (simmr_bam_emit(eng, &reads, &t, rec, total) != SIMMR_OK) return fail("--bam", simmr_last_error(eng));
    std::string e;
    OutFile f(a.bam, true);
    return bam_append_framed(eng, &mem, rec, total, &f) && (f.close(&e) || fail("--bam", e));
  }
  // --bam-sorted: the records of one range in coordinate order, with the key, the length and the end of each: a sorted run
  bool bam_sorted_range(simmr_engine* eng, const simmr_reads_out& reads, const simmr_truth_out& t, uint64_t n_reads, bool paired) {
    if (!*bam_sort && simmr_bam_sort_create(eng, bam_sort) != SIMMR_OK) return fail("--bam-sorted", simmr_last_error(eng));
    uint64_t total = 0;
    if (simmr_bam_sort_plan(*bam_sort, &sn, &reads, &t, n_reads, paired ? 1 : 0, &total) != SIMMR_OK) return fail("--bam-sorted", simmr_last_error(eng));
    DeviceMem mem;
    uint8_t* rec = nullptr;
    uint64_t *key = nullptr, *rec_off = nullptr;
    uint32_t* end = nullptr;
    std::vector<uint8_t> h;
    std::vector<uint64_t> off;
    std::vector<uint32_t> ends;
    SamSortedRun run;
    if (!(mem.alloc(&rec, total) && mem.alloc(&key, n_reads) && mem.alloc(&rec_off, n_reads + 1) && mem.alloc(&end, n_reads)))
      return fail("--bam-sorted", "device allocation failed");
    if (simmr_bam_sort_emit(*bam_sort, &reads, &t, rec, total, key, rec_off, end) != SIMMR_OK) return fail("--bam-sorted", simmr_last_error(eng));
    if (!(mem.fetch(&h, (const uint8_t*)rec, total) && mem.fetch(&run.key, (const uint64_t*)key, n_reads) && mem.fetch(&off, (const uint64_t*)rec_off, n_reads + 1) &&
          mem.fetch(&ends, (const uint32_t*)end, n_reads)))
      return fail("--bam-sorted", "copy back failed");
    run.len.resize(n_reads);
    for (uint64_t i = 0; i < n_reads; i++) run.len[i] = off[i + 1] - off[i];
    bam_ends.push_back(std::move(ends));
    std::string e;
    return bam_spill.add(std::move(run), std::move(h), &e) || fail("--bam-sorted", e);
  }
  // The file and its index.  Header and records are one stream: one range's records as they are, several merged by (key, range,
  // place in the range); the stream goes to the device in pieces of whole blocks (BgzfPieces carries the rest), so only the last
  // block is short.  The columns of the index take the same merge, as 16-byte tuples; they go up once, and simmr_bai_* writes
  // the index from them.
  bool finish_bam_sorted(simmr_engine* eng) {
    std::string e;
    if (!*bam_sort && simmr_bam_sort_create(eng, bam_sort) != SIMMR_OK) return fail("--bam-sorted", simmr_last_error(eng));
    const std::vector<SamSortedRun>& bam_runs = bam_spill.runs();
    uint64_t n = 0;
    for (const SamSortedRun& r : bam_runs) n += r.key.size();
    std::vector<uint64_t> key, rec_off(1, 0);
    std::vector<uint32_t> end;
    key.reserve(n); end.reserve(n); rec_off.reserve(n + 1);
    OutFile out(a.bam, false);
    BgzfPieces pieces(BAM_PIECE_BLOCKS, [&](const uint8_t* p, size_t bytes) {
      DeviceMem mem;
      uint8_t* src = nullptr;
      if (!mem.alloc(&src, bytes) || hipMemcpy(src, p, bytes, hipMemcpyHostToDevice) != hipSuccess) return fail("--bam-sorted", "copy to the device failed");
      return bam_append_framed(eng, &mem, src, bytes, &out) && out.ok();
    });
    if (!pieces.append(bam_head.data(), bam_head.size())) return false;
    if (!bam_spill.merge([&](const char* p, size_t len) { return pieces.append(p, len); }, &e)) return err.empty() && !e.empty() ? fail("--bam-sorted", e) : false;
    if (!bam_spill.spilled()) {
      if (!bam_runs.empty()) {
        key = bam_runs[0].key;
        end = bam_ends[0];
        for (uint64_t len : bam_runs[0].len) rec_off.push_back(rec_off.back() + len);
      }
    } else {
      // the columns: (key, end, length) of every record, 16 bytes, through the same merge
      std::vector<char> tuples(16 * n), order;
      std::vector<SamSortedRun> col_runs(bam_runs.size());
      uint64_t at = 0;
      for (size_t r = 0; r < bam_runs.size(); r++) {
        col_runs[r].key = bam_runs[r].key;
        col_runs[r].len.assign(bam_runs[r].key.size(), 16);
        col_runs[r].offset = 16 * at;
        for (size_t i = 0; i < bam_runs[r].key.size(); i++, at++) {
          const uint32_t len32 = (uint32_t)bam_runs[r].len[i];  // (a record is below 2^20 bytes)
          memcpy(&tuples[16 * at], &bam_runs[r].key[i], 8);
          memcpy(&tuples[16 * at + 8], &bam_ends[r][i], 4);
          memcpy(&tuples[16 * at + 12], &len32, 4);
        }
      }
      order.reserve(16 * n);
      const bool merged = sam_merge_sorted_runs(
          col_runs, [&](uint64_t from, size_t len, char* p) { if (from + len > tuples.size()) return false; memcpy(p, &tuples[from], len); return true; },
          [&](const char* p, size_t len) { order.insert(order.end(), p, p + len); return true; });
      if (!merged || order.size() != 16 * n) return fail("--bam-sorted", "the merge of the sorted ranges failed");
      for (uint64_t i = 0; i < n; i++) {
        uint64_t k; uint32_t en, len32;
        memcpy(&k, &order[16 * i], 8); memcpy(&en, &order[16 * i + 8], 4); memcpy(&len32, &order[16 * i + 12], 4);
        key.push_back(k); end.push_back(en); rec_off.push_back(rec_off.back() + len32);
      }
    }
    if (!pieces.finish()) return false;
    out.append(SIMMR_BGZF_EOF, SIMMR_BGZF_EOF_BYTES);
    if (!out.close(&e)) return fail("--bam-sorted", e);
    if (pieces.bytes() != bam_head.size() + rec_off.back()) return fail("--bam-sorted", "the merged stream and its columns disagree");
    // the index, from the columns
    DeviceMem mem;
    uint64_t *dkey = nullptr, *doff = nullptr, bai_bytes = 0;
    uint32_t* dend = nullptr;
    uint8_t* bai = nullptr;
    if (!(mem.alloc(&dkey, n) && mem.alloc(&dend, n) && mem.alloc(&doff, n + 1))) return fail("--bam-sorted", "device allocation failed");
    if ((n > 0 && (hipMemcpy(dkey, key.data(), n * 8, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dend, end.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess)) ||
        hipMemcpy(doff, rec_off.data(), (n + 1) * 8, hipMemcpyHostToDevice) != hipSuccess)
      return fail("--bam-sorted", "copy to the device failed");
    if (simmr_bai_plan(*bam_sort, dkey, dend, doff, n, bam_lengths.size(), bam_lengths.data(), bam_head.size(), &bai_bytes) != SIMMR_OK)
      return fail("--bam-sorted", simmr_last_error(eng));
    std::vector<uint8_t> h;
    if (!mem.alloc(&bai, bai_bytes)) return fail("--bam-sorted", "device allocation failed");
    if (simmr_bai_emit(*bam_sort, bai, bai_bytes) != SIMMR_OK) return fail("--bam-sorted", simmr_last_error(eng));
    if (!mem.fetch(&h, (const uint8_t*)bai, bai_bytes)) return fail("--bam-sorted", "copy back failed");
    OutFile index(bam_index_path(), false);
    index.append(h.data(), h.size());
    return index.close(&e) || fail("--bam-index", e);
  }
  // the end-of-file block behind the last range's blocks
  bool finish_bam() {
    std::string e;
    OutFile f(a.bam, true);
    f.append(SIMMR_BGZF_EOF, SIMMR_BGZF_EOF_BYTES);
    return f.close(&e) || fail("--bam", e);
  }
  // the alignment lines of one range, formatted on the device from its columns and truth columns, appended to the file
  bool sam_range(simmr_engine* eng, const simmr_reads_out& reads, const simmr_truth_out& t, uint64_t n_reads, bool paired) {
    uint64_t total = 0;
    if (a.sam_sorted) return sam_sorted_range(eng, reads, t, n_reads, paired);
    if (simmr_sam_plan(eng, &sn, &reads, &t, n_reads, paired ? 1 : 0, &total) != SIMMR_OK) return fail("--sam", simmr_last_error(eng));
    DeviceMem mem;
    uint8_t* text = nullptr;
    std::vector<uint8_t> h;
    if (!mem.alloc(&text, total)) return fail("--sam", "device allocation failed");
    if (simmr_sam_emit(eng, &reads, &t, text, total) != SIMMR_OK) return fail("--sam", simmr_last_error(eng));
    if (!mem.fetch(&h, text, total)) return fail("--sam", "copy back failed");
    std::string e;
    OutFile f(a.sam, true);
    f.append(h.data(), h.size());
    return f.close(&e) || fail("--sam", e);
  }
  // the same lines in coordinate order, with the key and the length of each: a sorted run for finish() to merge
  bool sam_sorted_range(simmr_engine* eng, const simmr_reads_out& reads, const simmr_truth_out& t, uint64_t n_reads, bool paired) {
    uint64_t total = 0;
    if (simmr_sam_sort_plan(eng, &sn, &reads, &t, n_reads, paired ? 1 : 0, &total) != SIMMR_OK) return fail("--sam-sorted", simmr_last_error(eng));
    DeviceMem mem;
    uint8_t* text = nullptr;
    uint64_t *key = nullptr, *line_off = nullptr;
    std::vector<uint8_t> h;
    std::vector<uint64_t> off;
    SamSortedRun run;
    if (!(mem.alloc(&text, total) && mem.alloc(&key, n_reads) && mem.alloc(&line_off, n_reads + 1))) return fail("--sam-sorted", "device allocation failed");
    if (simmr_sam_sort_emit(eng, &reads, &t, text, total, key, line_off) != SIMMR_OK) return fail("--sam-sorted", simmr_last_error(eng));
    if (!(mem.fetch(&h, text, total) && mem.fetch(&run.key, key, n_reads) && mem.fetch(&off, line_off, n_reads + 1))) return fail("--sam-sorted", "copy back failed");
    run.len.resize(n_reads);
    for (uint64_t i = 0; i < n_reads; i++) run.len[i] = off[i + 1] - off[i];
    std::string e;
    return sam_spill.add(std::move(run), std::move(h), &e) || fail("--sam-sorted", e);
  }
  // the run's lines behind the header: one range's text as it is, several merged by (key, range, place in the range)
  bool finish_sam_sorted() {
    std::string e, merge_err;
    OutFile out(a.sam, true);
    const bool merged = sam_spill.merge([&](const char* p, size_t n) { out.append(p, n); return out.ok(); }, &merge_err);
    if (!out.close(&e)) return fail("--sam-sorted", e);
    return merged || fail("--sam-sorted", merge_err);
  }
  // the kept sites go up as one list — genome index, contig, pos: ascending, genome by genome — and the table starts at zero
  bool begin_pileup(simmr_engine* eng) {
    DeviceMem mem;
    simmr_pileup_sites s{};
    s.n = sites.pos.size();
    uint32_t *g = nullptr, *c = nullptr;
    uint64_t* p = nullptr;
    if (!(mem.alloc(&g, s.n) && mem.alloc(&c, s.n) && mem.alloc(&p, s.n))) return fail("--strain-vcf", "device allocation failed");
    if (s.n > 0 && (hipMemcpy(g, site_genome.data(), s.n * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(c, sites.contig.data(), s.n * 4, hipMemcpyHostToDevice) != hipSuccess ||
                    hipMemcpy(p, sites.pos.data(), s.n * 8, hipMemcpyHostToDevice) != hipSuccess)) return fail("--strain-vcf", "copy to the device failed");
    s.genome = g; s.contig = c; s.pos = p;
    return simmr_pileup_reset(eng, &s) == SIMMR_OK || fail("--strain-vcf", simmr_last_error(eng));
  }
  // every range adds to the run's tables (enqueued behind the emit; the copies that follow wait for the device)
  bool add_range(simmr_engine* eng, const simmr_reads_out& reads, uint64_t n_reads, bool paired) {
    if (!a.stats.empty() && simmr_stats_add(eng, &reads, n_reads, paired ? 2u : 1u) != SIMMR_OK) return fail("--stats", simmr_last_error(eng));
    if (fit() && simmr_fit_add(eng, &reads, n_reads, paired ? 2u : 1u) != SIMMR_OK) return fail("--fit-model", simmr_last_error(eng));
    if (depth() && simmr_depth_add(eng, &reads, n_reads) != SIMMR_OK) return fail("--depth", simmr_last_error(eng));
    if (vcf() && simmr_pileup_add(eng, &reads, n_reads) != SIMMR_OK) return fail("--strain-vcf", simmr_last_error(eng));
    if (overlaps() && simmr_overlap_add(eng, &reads, n_reads) != SIMMR_OK) return fail("--overlaps", simmr_last_error(eng));
    std::string e;
    qual_offset = reads.qual_offset;
    if (a.truth.empty() && !sam() && !bam()) return true;
    DeviceMem mem;  // the truth columns on the device: --truth copies them out, --sam and --bam format from them
    simmr_truth_out t{};
    if (!device_truth(eng, &reads, n_reads, &mem, &t, a.truth.empty() ? nullptr : &truth, &e)) return fail(!a.truth.empty() ? "--truth" : sam() ? "--sam" : "--bam", e);
    if (bam() && !(a.bam_sorted ? bam_sorted_range(eng, reads, t, n_reads, paired) : bam_range(eng, reads, t, n_reads, paired))) return false;
    return !sam() || sam_range(eng, reads, t, n_reads, paired);
  }
  bool write_range(const std::vector<Genome>& genomes, const HostReads& h) {
    std::string e;
    return a.truth.empty() || write_truth_tsv(genomes, h, truth, qual_offset, a.truth, false, &e) || fail("--truth", e);
  }
  // the overlaps of every range added: one plan, then window by window through the file — a window is what the text buffer of
  // the FASTQ drain holds (a place whose records alone are more than that gets a buffer of its own size)
  bool finish_overlaps(simmr_engine* eng) {
    uint64_t n = 0, pairs = 0, total = 0;
    if (simmr_overlap_plan(eng, a.min_overlap, &n, &pairs, &total) != SIMMR_OK) return fail("--overlaps", simmr_last_error(eng));
    std::string e;
    OutFile f(a.overlaps, false);
    GrowBuf text;
    std::vector<uint8_t> h;
    uint64_t room = std::min<uint64_t>(total, TEXT_CHUNK);
    for (uint64_t place = 0; place < n;) {
      uint64_t n_places = 0, n_rec = 0, bytes = 0;
      const int rc = simmr_overlap_window(eng, place, room, &n_places, &n_rec, &bytes);
      if (rc == SIMMR_ERANGE && bytes > room) { room = bytes; continue; }
      if (rc != SIMMR_OK) return fail("--overlaps", simmr_last_error(eng));
      uint8_t* dst = text.room(std::max<uint64_t>(bytes, 1));
      if (!dst) return fail("--overlaps", "device allocation failed");
      if (simmr_overlap_emit(eng, place, n_places, nullptr, dst, bytes) != SIMMR_OK) return fail("--overlaps", simmr_last_error(eng));
      if (!DeviceMem::fetch(&h, (const uint8_t*)dst, bytes)) return fail("--overlaps", "copy back failed");
      f.append(h.data(), h.size());
      if (!f.ok()) break;
      place += n_places;
    }
    return f.close(&e) || fail("--overlaps", e);
  }
  // the model of every range added: one plan, the columns through device buffers of the planned sizes, the bincode image
  static constexpr uint64_t FIT_PAIR_CAPACITY = 1ull << 24;  // distinct changed (reference, alternate) pairs a run may show
  bool finish_fit(simmr_engine* eng) {
    simmr_fit_info f{};
    if (simmr_fit_plan(eng, &f) != SIMMR_OK) return fail("--fit-model", simmr_last_error(eng));
    DeviceMem mem;
    simmr_fit_out d{}, h{};
    d.ref_capacity = f.n_ref_kmers; d.pair_capacity = f.n_pairs; d.position_capacity = f.n_positions;
    d.length_bin_capacity = f.n_length_bins; d.insert_bin_capacity = f.n_insert_bins;
    if (!(mem.alloc(&d.kmer_ref, f.n_ref_kmers) && mem.alloc(&d.kmer_first, f.n_ref_kmers + 1) && mem.alloc(&d.pair_alt, f.n_pairs) &&
          mem.alloc(&d.pair_prob, f.n_pairs) && mem.alloc(&d.qual_density, f.n_positions * SIMMR_FIT_DENSITIES) &&
          mem.alloc(&d.length_density, f.n_length_bins) && mem.alloc(&d.length_lo, f.n_length_bins) && mem.alloc(&d.length_hi, f.n_length_bins) &&
          mem.alloc(&d.insert_density, f.n_insert_bins) && mem.alloc(&d.insert_lo, f.n_insert_bins) && mem.alloc(&d.insert_hi, f.n_insert_bins)))
      return fail("--fit-model", "device allocation failed");
    if (simmr_fit_emit(eng, &d) != SIMMR_OK) return fail("--fit-model", simmr_last_error(eng));
    std::vector<uint32_t> kmer_ref, pair_alt, llo, lhi, ilo, ihi;
    std::vector<uint64_t> kmer_first;
    std::vector<float> pair_prob;
    std::vector<double> qd, ld, id;
    if (!(DeviceMem::fetch(&kmer_ref, (const uint32_t*)d.kmer_ref, f.n_ref_kmers) && DeviceMem::fetch(&kmer_first, (const uint64_t*)d.kmer_first, f.n_ref_kmers + 1) &&
          DeviceMem::fetch(&pair_alt, (const uint32_t*)d.pair_alt, f.n_pairs) && DeviceMem::fetch(&pair_prob, (const float*)d.pair_prob, f.n_pairs) &&
          DeviceMem::fetch(&qd, (const double*)d.qual_density, f.n_positions * SIMMR_FIT_DENSITIES) &&
          DeviceMem::fetch(&ld, (const double*)d.length_density, f.n_length_bins) && DeviceMem::fetch(&llo, (const uint32_t*)d.length_lo, f.n_length_bins) &&
          DeviceMem::fetch(&lhi, (const uint32_t*)d.length_hi, f.n_length_bins) && DeviceMem::fetch(&id, (const double*)d.insert_density, f.n_insert_bins) &&
          DeviceMem::fetch(&ilo, (const uint32_t*)d.insert_lo, f.n_insert_bins) && DeviceMem::fetch(&ihi, (const uint32_t*)d.insert_hi, f.n_insert_bins)))
      return fail("--fit-model", "copy back failed");
    h.kmer_ref = kmer_ref.data(); h.kmer_first = kmer_first.data(); h.pair_alt = pair_alt.data(); h.pair_prob = pair_prob.data();
    h.qual_density = qd.data(); h.length_density = ld.data(); h.length_lo = llo.data(); h.length_hi = lhi.data();
    h.insert_density = id.data(); h.insert_lo = ilo.data(); h.insert_hi = ihi.data();
    std::string e;
    return write_fit_model(f, h, a.fit_model, &e) || fail("--fit-model", e);
  }
  bool finish(simmr_engine* eng, const std::vector<Genome>& genomes) {
    std::string e;
    if (fit() && !finish_fit(eng)) return false;
    if (overlaps() && !finish_overlaps(eng)) return false;
    if (sam() && a.sam_sorted && !finish_sam_sorted()) return false;
    if (bam() && !(a.bam_sorted ? finish_bam_sorted(eng) : finish_bam())) return false;
    if (!a.stats.empty()) {
      auto st = std::make_unique<simmr_run_stats>();
      if (simmr_stats_read(eng, st.get()) != SIMMR_OK) return fail("--stats", simmr_last_error(eng));
      if (!write_stats_tsv(*st, a.stats, &e)) return fail("--stats", e);
    }
    if (depth_files() && !write_depth_files(eng, a, genomes, depth_positions, depth_contigs, &e)) return fail("--depth", e);
    if (gold() && !write_gold_files(eng, a, genomes, depth_positions, &e)) return fail("--gold-assembly", e);
    return !vcf() || write_vcf_file(eng, a, genomes, sites, site_genome, depth_positions, &e) || fail("--strain-vcf", e);
  }
};

// ---- output of one planned range ------------------------------------------------------------------------------------
// A run is generated range by range of its units (pairs / long reads): the reference holds every read of a run in RAM
// before it writes (main.rs:180-206, readme.md:219-220); here a range is what fits the device next to the reference
// (--device-chunk-reads, or a share of the free memory), and the FASTQ text of range k is copied out and written
// while range k + 1 is planned and emitted.  The text of a range comes straight from its plan
// (simmr_fastq_plan_direct / simmr_emit_fastq: no SoA columns in between).
struct TextDrain {
  // two device buffers for the text and two pinned buffers for the copy out; the file is appended to in order
  GrowBuf dev[2];  // (a buffer is free again when it is asked for: its previous text was drained two ranges ago)
  uint64_t len[2] = {0, 0};
  void* pin[2] = {nullptr, nullptr};
  hipStream_t cs = nullptr;
  hipEvent_t emitted = nullptr;
  std::optional<OutFile> f;
  static constexpr size_t CHUNK = TEXT_CHUNK;
  int pending = -1;  // buffer whose text still has to go to the file
  bool open(const std::string& output, std::string* err) {
    f.emplace(output, true);
    if (!f->ok()) { *err = f->error(); return false; }
    if (hipHostMalloc(&pin[0], CHUNK, hipHostMallocDefault) != hipSuccess || hipHostMalloc(&pin[1], CHUNK, hipHostMallocDefault) != hipSuccess ||
        hipStreamCreateWithFlags(&cs, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&emitted, hipEventDisableTiming) != hipSuccess) { *err = "pinned buffer / stream allocation failed"; return false; }
    return true;
  }
  // the text in buffer b (written by work queued on the null stream up to now) goes to the file; returns at once after
  // queueing the first copy, the rest happens in flush()
  bool submit(int b, uint64_t bytes, std::string* err) {
    if (!flush(err)) return false;
    len[b] = bytes;
    if (hipEventRecord(emitted, nullptr) != hipSuccess || hipStreamWaitEvent(cs, emitted, 0) != hipSuccess) { *err = "event failed"; return false; }
    if (bytes > 0 && hipMemcpyAsync(pin[0], dev[b].p, std::min<uint64_t>(CHUNK, bytes), hipMemcpyDeviceToHost, cs) != hipSuccess) { *err = "copy back failed"; return false; }
    pending = b;
    return true;
  }
  // write the pending text: the copy of chunk i + 1 runs while chunk i is written to the file
  bool flush(std::string* err) {
    if (pending < 0) return true;
    const int b = pending;
    pending = -1;
    const uint64_t total = len[b], n_chunks = (total + CHUNK - 1) / CHUNK;
    auto len_of = [&](uint64_t i) { return (size_t)std::min<uint64_t>(CHUNK, total - i * CHUNK); };
    for (uint64_t i = 0; i < n_chunks; i++) {
      if (hipStreamSynchronize(cs) != hipSuccess) { *err = "copy back failed"; return false; }  // chunk i is in pin[i & 1]
      if (i + 1 < n_chunks && hipMemcpyAsync(pin[(i + 1) & 1], (const char*)dev[b].p + (i + 1) * CHUNK, len_of(i + 1), hipMemcpyDeviceToHost, cs) != hipSuccess) { *err = "copy back failed"; return false; }
      f->append(pin[i & 1], len_of(i));
      if (!f->ok()) { *err = f->error(); return false; }
    }
    return true;
  }
  // the pending text, then the file's one status
  bool close(std::string* err) { return flush(err) && f->close(err); }
  ~TextDrain() {
    if (cs) (void)hipStreamDestroy(cs);
    if (emitted) (void)hipEventDestroy(emitted);
    for (void* q : pin) if (q) (void)hipHostFree(q);
  }
};

// One scope of the run = one plan function over a range of units: all genomes' pairs in one plan, one genome's pairs
// (custom profiles), or all long reads.
struct Scope {
  enum Kind { PE_ALL, PE_GENOME, LONG } kind;
  std::vector<uint32_t> idx;    // the scope's genomes, ascending
  std::vector<uint64_t> reads;  // reads asked of each, in generation order
  simmr_error_profile pod;
  int has_seed;
  uint64_t seed;  // (of --seed, or the one probe_scope drew)
  uint32_t id_base;
  uint64_t text_bytes_per_unit;  // what sizes the ranges; an upper estimate of a unit's FASTQ text
  bool paired() const { return kind != LONG; }
  uint32_t reads_per_unit() const { return paired() ? 2u : 1u; }
  uint64_t units(size_t k) const { return reads[k] / reads_per_unit(); }  // simulate.rs:179: a genome's odd read makes no pair
  // plans units [first, first + count) of the scope; SIMMR_* code
  int plan(simmr_engine* en, simmr_range rg, simmr_plan_info* pi) const {
    switch (kind) {
      case PE_ALL: return simmr_pe_plan_multi(en, (uint32_t)idx.size(), idx.data(), reads.data(), &pod, has_seed, seed, rg, pi);
      case PE_GENOME: return simmr_pe_plan(en, idx[0], &pod, reads[0], has_seed, seed, rg, pi);
      case LONG: return simmr_long_plan(en, (uint32_t)idx.size(), idx.data(), reads.data(), &pod, has_seed, seed, rg, pi);
    }
    return SIMMR_EINVAL;
  }
  // columns (host writer only)
  int emit(simmr_engine* en, const simmr_reads_out* o) const { return paired() ? simmr_pe_emit(en, id_base, o) : simmr_long_emit(en, id_base, o); }
};

// Plans an empty range of the scope.  The answer says whether the library takes this plan at all (SIMMR_ENOTSUP: a custom
// profile in the one plan over all genomes).  Without --seed the call draws a seed, and it becomes the scope's: every
// plan call would draw its own otherwise (simulate.rs:174), and the ranges have to continue one stream.
static int probe_scope(simmr_engine* eng, Scope* sc) {
  simmr_plan_info p0{};
  const int rc = sc->plan(eng, simmr_range{0, 0}, &p0);
  if (rc == SIMMR_OK && !sc->has_seed) {
    sc->has_seed = 1; sc->seed = p0.seed_used;
    // (without --seed the library selects per-read lengths by itself; the ranges, which now name a seed, say so)
    if (!sc->paired()) sc->pod.length_mode = SIMMR_LEN_PER_READ;
  }
  return rc;
}

struct NameTables {  // simmr_fastq_names of the scope's genomes
  std::vector<uint32_t> ncontigs;
  std::vector<const char*> gids, sids;
  simmr_fastq_names names{};
  NameTables(const std::vector<Genome>& genomes, const Scope& sc) {
    for (uint32_t gi : sc.idx) {
      gids.push_back(genomes[gi].uuid.c_str());
      ncontigs.push_back((uint32_t)genomes[gi].sequence.size());
      for (const Seq& s : genomes[gi].sequence) sids.push_back(s.id.c_str());
    }
    names = simmr_fastq_names{(uint32_t)sc.idx.size(), sc.idx.data(), gids.data(), ncontigs.data(), sids.data()};
  }
};

// The ranges of a scope, the same whoever walks them: `chunk_units` each (0: all in one).  Several engines get at least a
// range each, of at most MAX_TEXT bytes of text (a range waits in pinned host memory for its turn; allocating that costs
// ~0.25 s per GB, once).  A scope without a unit has one empty range.
struct Ranges {
  static constexpr uint64_t MAX_TEXT = 1ull << 30;
  uint64_t total = 0, chunk, n;
  Ranges(const Scope& sc, uint64_t chunk_units, size_t n_engines) : chunk(chunk_units) {
    for (size_t k = 0; k < sc.reads.size(); k++) total += sc.units(k);
    if (chunk == 0 || chunk > total) chunk = total;
    if (n_engines > 1) chunk = std::min({chunk, (total + n_engines - 1) / n_engines, MAX_TEXT / std::max<uint64_t>(sc.text_bytes_per_unit, 1)});
    chunk = std::max<uint64_t>(chunk, 1);
    n = std::max<uint64_t>((total + chunk - 1) / chunk, 1);
  }
  simmr_range at(uint64_t k) const { return simmr_range{k * chunk, std::min(chunk, total - k * chunk)}; }
};

// Plans range rg of the scope on `eng` and, given the names, sizes its FASTQ text.  SIMMR_OK with *bytes; SIMMR_ENOTSUP if
// the headers need the host writer (an id with a brace, a header over 255 bytes: the range stays planned; the plan itself
// answers this code only to probe_scope); or the code of the call that failed, with simmr_last_error.
static int plan_range(simmr_engine* eng, const Scope& sc, simmr_range rg, const NameTables* nt, const std::string& header_format,
                      simmr_plan_info* pi, uint64_t* bytes) {
  const int rc = sc.plan(eng, rg, pi);  // the reference unwrap()s this Err (simulate.rs:137)
  if (rc != SIMMR_OK || !nt) return rc;
  return simmr_fastq_plan_direct(eng, header_format.c_str(), &nt->names, sc.id_base, bytes);
}

// Generates the scope range by range and appends its FASTQ to args.output.  0, or 1 after die().
static int run_scope(simmr_engine* eng, const CliArgs& args, const std::vector<Genome>& genomes, const Scope& sc, uint64_t chunk_units,
                     SideOutputs* side) {
  const Ranges ranges(sc, chunk_units, 1);
  const uint32_t rpu = sc.reads_per_unit();
  NameTables nt(genomes, sc);
  std::string err;
  bool use_device_text = !args.host_fastq && !side->wanted();
  uint64_t text_bytes = 0, n_passes = 0;
  TextDrain drain;
  if (use_device_text && !drain.open(args.output, &err)) return die(err);
  int buf = 0;
  for (uint64_t k = 0; k < ranges.n; k++) {
    const simmr_range rg = ranges.at(k);
    simmr_plan_info pi{};
    uint64_t bytes = 0;
    const int rc = plan_range(eng, sc, rg, use_device_text ? &nt : nullptr, args.read_header_format, &pi, &bytes);
    if (rc == SIMMR_ENOTSUP) {
      use_device_text = false;  // the host writer frames this run from here
      if (!drain.close(&err)) return die(err);
    } else if (rc != SIMMR_OK) {
      return die(simmr_last_error(eng));
    }
    if (use_device_text) {
      // (no text: a scope without a unit — --num-reads < 2, a genome whose share is below one pair: the reference writes
      // nothing for it and goes on, simulate.rs:179, main.rs:188-206)
      if (bytes == 0) continue;
      uint8_t* dst = drain.dev[buf].room(bytes);
      if (!dst) return die("no device memory for " + std::to_string(bytes) + " bytes of FASTQ text: use a smaller --device-chunk-reads");
      if (simmr_emit_fastq(eng, dst, bytes) != SIMMR_OK) return die(simmr_last_error(eng));
      if (!drain.submit(buf, bytes, &err)) reads_not_written(err);
      buf ^= 1;
      text_bytes += bytes;
      n_passes++;
      continue;
    }
    // columns to the host, framed by the restatement of fastq.rs in host.cpp, genome by genome
    DeviceOut d;
    if (!d.init(pi.n_reads, pi.total_bases, pi.slot_bytes)) return die("device allocation failed");
    if (sc.emit(eng, &d.o) != SIMMR_OK) return die(simmr_last_error(eng));
    if (!side->add_range(eng, d.o, pi.n_reads, sc.paired())) return die(side->err);
    HostReads h;
    if (!d.to_host(pi.n_reads, pi.total_bases, sc.paired(), &h)) return die("copy back failed");
    if (!side->write_range(genomes, h)) return die(side->err);
    uint64_t g_first = 0;  // first unit of genome idx[j] in the scope
    for (size_t j = 0; j < sc.idx.size(); j++) {
      const Genome& g = genomes[sc.idx[j]];
      const uint64_t lo = std::max(rg.first, g_first), hi = std::min(rg.first + rg.count, g_first + sc.units(j));
      if (hi > lo && !write_to_fastq(g.uuid, g, h, (lo - rg.first) * rpu, (hi - lo) * rpu, args.output, args.read_header_format, true, &err))
        reads_not_written(err);
      g_first += sc.units(j);
    }
  }
  if (use_device_text && !drain.close(&err)) reads_not_written(err);
  if (n_passes > 1)
    info(std::to_string(ranges.total * rpu) + " reads in " + std::to_string(n_passes) + " device passes, " + std::to_string(text_bytes) + " bytes of FASTQ");
  return 0;
}

// ---- the same over several engines (--devices a,b,...): the whole node behind the reference's one call ------------------
// The reference's product is one call that writes one FASTQ (main.rs:180-206).  Here the scope's ranges — the same ranges
// run_scope walks, whose text does not depend on how the run is cut (tests/test_gpu_cli.py) — are dealt to the engines in
// turn: engine d plans and emits ranges d, d + N, d + 2N, ... on a host thread of its own (one engine per device, or
// several on one: an ordinal may repeat), copies each range's text to pinned host memory over ITS device's link as soon as
// it is emitted — the devices' copies run side by side; a drain that waited for its turn would put the whole node behind one
// PCIe link — and appends it to the file when the range before it is on disk.  Ids are
// those of the single-engine run (the library's ids come from the global unit index, simulate.rs:85-89); nothing is
// exchanged between devices, the run counters are not needed for the files.  0, or 1 after die().
static int run_scope_devices(const std::vector<simmr_engine*>& engs, const std::vector<int>& ordinals, const CliArgs& args,
                             const std::vector<Genome>& genomes, const Scope& sc, uint64_t chunk_units) {
  const size_t N = engs.size();
  const Ranges ranges(sc, chunk_units, N);
  if (ranges.total == 0) return 0;  // (the reference writes nothing for a scope without a unit)
  OutFile f(args.output, true);
  if (!f.ok()) return die(f.error());
  std::mutex m;
  std::condition_variable cv;
  uint64_t turn = 0;        // the range whose text goes to the file next
  bool failed = false;
  std::string first_error;
  uint64_t text_bytes = 0;
  auto fail = [&](const std::string& what) {
    std::lock_guard<std::mutex> lk(m);
    if (!failed) { failed = true; first_error = what; }
    cv.notify_all();
  };
  auto worker = [&](size_t d) {
    simmr_engine* eng = engs[d];
    if (hipSetDevice(ordinals[d]) != hipSuccess) return fail("hipSetDevice failed");
    NameTables nt(genomes, sc);
    // this engine's text buffers: one on the device, one pinned on the host (both grow to the largest range), a copy stream
    struct Bufs {
      GrowBuf dev, host{true};
      hipStream_t cs = nullptr;
      ~Bufs() { if (cs) (void)hipStreamDestroy(cs); }
    } b;
    if (hipStreamCreateWithFlags(&b.cs, hipStreamNonBlocking) != hipSuccess) return fail("stream allocation failed");
    for (uint64_t k = d; k < ranges.n; k += N) {
      { std::lock_guard<std::mutex> lk(m); if (failed) return; }
      simmr_plan_info pi{};
      uint64_t bytes = 0;
      const int rc = plan_range(eng, sc, ranges.at(k), &nt, args.read_header_format, &pi, &bytes);
      if (rc == SIMMR_ENOTSUP) return fail(std::string("--devices writes the text on the devices, and this run's headers need the host writer (") + simmr_last_error(eng) + "): use --device with --host-fastq");
      if (rc != SIMMR_OK) return fail(simmr_last_error(eng));
      if (bytes) {
        if (!b.dev.room(bytes)) return fail("no device memory for " + std::to_string(bytes) + " bytes of FASTQ text: use a smaller --device-chunk-reads");
        if (!b.host.room(bytes)) return fail("no pinned host memory for " + std::to_string(bytes) + " bytes of FASTQ text");
        if (simmr_emit_fastq(eng, (uint8_t*)b.dev.p, bytes) != SIMMR_OK) return fail(simmr_last_error(eng));
        // over this device's own link, now: the emit ran on the null stream of the device, the copy stream waits for it
        hipEvent_t done = nullptr;
        if (hipEventCreateWithFlags(&done, hipEventDisableTiming) != hipSuccess || hipEventRecord(done, nullptr) != hipSuccess ||
            hipStreamWaitEvent(b.cs, done, 0) != hipSuccess ||
            hipMemcpyAsync(b.host.p, b.dev.p, bytes, hipMemcpyDeviceToHost, b.cs) != hipSuccess || hipStreamSynchronize(b.cs) != hipSuccess) {
          if (done) (void)hipEventDestroy(done);
          return fail("copy back failed");
        }
        (void)hipEventDestroy(done);
      }
      {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return failed || turn == k; });
        if (failed) return;
      }
      f.append(b.host.p, bytes);  // this thread owns the file until it passes the turn on
      const bool ok = f.ok();
      {
        std::lock_guard<std::mutex> lk(m);
        if (!ok && !failed) { failed = true; first_error = "Failed to write reads to the output file: " + f.error(); }
        text_bytes += bytes;
        turn = k + 1;
      }
      cv.notify_all();
      if (!ok) return;
    }
  };
  std::vector<std::thread> threads;
  for (size_t d = 0; d < N; d++) threads.emplace_back(worker, d);
  for (auto& t : threads) t.join();
  std::string err;
  if (!f.close(&err) && !failed) { failed = true; first_error = "Failed to write reads to the output file: " + err; }
  if (failed) return die(first_error);
  info(std::to_string(ranges.total * sc.reads_per_unit()) + " reads in " + std::to_string(ranges.n) + " device passes on " + std::to_string(N) +
       " engines, " + std::to_string(text_bytes) + " bytes of FASTQ");
  return 0;
}

// units per range when --device-chunk-reads is not given: what a third of the free device memory holds, at
// `text_bytes_per_unit` of FASTQ text (two buffers) plus the plan's columns per unit
static uint64_t auto_chunk_units(uint64_t text_bytes_per_unit) {
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return 0;
  const uint64_t per_unit = 2 * text_bytes_per_unit + 96;
  return std::max<uint64_t>((uint64_t)free_b / 3 / per_unit, 1024);
}

// Genome::from_fasta (genome.rs:89-162) with the sequences going straight to the device: the host only finds
// the records; simmr_stage_fasta normalises (needletail normalize(false), genome.rs:114), applies the size filter
// of main.rs:117-162 and packs.  Returns 1 if the genome has no usable sequence (it is left out), -1 on error.
static int load_genome_device(simmr_engine* eng, uint32_t slot, const std::string& path, bool contiguous, uint64_t min_size,
                              Genome* g, std::string* err) {
  FastaRecords recs;
  if (!scan_fasta(path, &recs, err)) return -1;
  const uint32_t n = (uint32_t)recs.ids.size();
  std::vector<const uint8_t*> body(n);
  std::vector<uint64_t> len(n), count(n);
  for (uint32_t c = 0; c < n; c++) { body[c] = (const uint8_t*)recs.data.data() + recs.body[c].first; len[c] = recs.body[c].second; }
  uint32_t n_staged = 0;
  if (simmr_stage_fasta(eng, slot, n, body.data(), len.data(), contiguous ? 1 : 0, contiguous ? 0 : min_size, count.data(),
                        &n_staged) != SIMMR_OK) {
    *err = simmr_last_error(eng);
    return -1;
  }
  g->uuid = uuid_from_u64(generate_id());  // genome.rs:124,140
  g->filepath = path;
  g->contiguous = contiguous;
  g->size = 0;
  for (uint32_t c = 0; c < n; c++) g->size += count[c];
  g->sequence.clear();
  if (contiguous) {  // genome.rs:121-137
    Seq whole;
    whole.id = "whole genome";
    whole.uuid = generate_id();
    whole.size = g->size;
    g->sequence.push_back(std::move(whole));
  } else {
    for (uint32_t c = 0; c < n; c++) {
      if (count[c] <= min_size) {
        warn("(" + path + ") Sequence " + recs.ids[c] + " doesn't meet size requirements, size = " + std::to_string(count[c]) +
             ", min size = " + std::to_string(min_size));
        continue;
      }
      Seq q;
      q.id = recs.ids[c];
      q.uuid = generate_id();
      q.size = count[c];
      g->sequence.push_back(std::move(q));
    }
  }
  g->num_seqs = g->sequence.size();
  if (n_staged == 0) { warn("Removing " + path + " from simulation, it doesn't have usable sequences"); return 1; }
  return 0;
}

// `--fit-from-sam FILE --fit-model OUT`: no simulation.  Every piece of the file is one simmr_fit_add_sam; then the plan and the
// model file of --fit-model.  What was taken and skipped is printed in the manner of the reference's "Skipped N alignments ..."
// lines (simmrd/src/main.rs:259-290).
static int run_fit_from_sam(const CliArgs& args) {
  if (int rc = probe_file("--fit-from-sam", args.fit_from_sam)) return rc;
  Engines engines;
  simmr_engine* eng = nullptr;
  if (simmr_engine_create(args.device, &eng) != SIMMR_OK) return die(std::string("cannot create engine: ") + simmr_last_error(nullptr));
  engines.v.push_back(eng);
  SideOutputs side(args);
  if (is_regular_file(args.fit_model)) remove(args.fit_model.c_str());
  if (simmr_fit_reset(eng, args.fit_k, args.fit_max_alt, SideOutputs::FIT_PAIR_CAPACITY) != SIMMR_OK) return die(std::string("--fit-model: ") + simmr_last_error(eng));
  info("Parsing " + args.fit_from_sam);
  const uint32_t n_sets = args.single_reads ? 1u : 2u;
  float device_ms = 0;
  if (int rc = file_pieces("--fit-from-sam", args.fit_from_sam, PieceCut{PieceCut::Newline, 1}, [&](const uint8_t* d, const char*, size_t bytes) {
        if (simmr_fit_add_sam(eng, d, bytes, n_sets) != SIMMR_OK) return die(std::string("--fit-from-sam: ") + simmr_last_error(eng));
        float ms = 0;  // (synchronises: the buffer is free for the next piece)
        if (simmr_last_fit_ms(eng, &ms) != SIMMR_OK) return die(std::string("--fit-from-sam: ") + simmr_last_error(eng));
        device_ms += ms;
        return 0;
      }))
    return rc;
  simmr_fit_sam_counts c{};
  if (simmr_fit_sam_counts_read(eng, &c) != SIMMR_OK) return die(std::string("--fit-from-sam: ") + simmr_last_error(eng));
  info("Read " + n(c.lines) + " lines: " + n(c.header_lines) + " header lines, " + n(c.records) + " alignments");
  info("Using " + n(c.taken_alignment) + " alignments (" + n(c.taken_quality) + " for read lengths and qualities)");
  info("Skipped " + n(c.skip_no_sequence) + " alignments that were missing sequences");
  info("Skipped " + n(c.skip_secondary) + " alignments that were secondary or supplementary");
  info("Skipped " + n(c.skip_too_long) + " alignments with reads longer than " + n(SIMMR_FIT_MAX_L) + " bases");
  info("Skipped " + n(c.skip_unmapped) + " alignments where the read was unmapped");
  info("Skipped " + n(c.skip_mapq0) + " alignments with MAPQ == 0");
  info("Skipped " + n(c.skip_mate_unmapped) + " alignments where the mate was unmapped");
  info("Skipped " + n(c.skip_no_md) + " alignments without an MD tag");
  info("Skipped " + n(c.skip_insert) + " alignments with an insert size above " + n(SIMMR_FIT_MAX_INSERT));
  info("Skipped " + n(c.skip_cigar_op) + " alignments with a CIGAR of * or an operation other than M = X I D S H");
  info("Skipped " + n(c.skip_inconsistent) + " alignments whose CIGAR, MD and sequence disagree");
  if (!side.finish_fit(eng)) return die(side.err);
  info("Wrote sequence error model to " + args.fit_model);
  return 0;
}

static int run_main(int argc, char** argv) {
  CliArgs args;
  std::string err;
  bool help = false;
  if (!parse_cli_args(argc, argv, &args, &err, &help)) { fprintf(stderr, "error: %s\n\n%s", err.c_str(), usage().c_str()); return 2; }
  if (help) { fputs(usage().c_str(), stdout); return 0; }
  if (!args.fit_from_sam.empty()) return run_fit_from_sam(args);
  if (!args.eval_sam.empty()) return run_eval_sam(args);
  if (!args.eval_overlaps.empty()) return run_eval_overlaps(args);
  if (!args.eval_vcf.empty()) return run_eval_vcf(args);
  if (!args.eval_classified.empty()) return run_eval_classified(args);
  if (!args.eval_assembly.empty()) return run_eval_assembly(args);
  if (!args.eval_placement.empty()) return run_eval_placement(args);
  if (!args.eval_bins.empty()) return run_eval_bins(args);
  if (!args.eval_corrected.empty()) return run_eval_corrected(args);

  SideOutputs side(args);
  if (side.refuse_devices()) return die(side.err);
  if ((side.sam() || side.bam()) && !sam_check_names(args, &err)) return die(err);
  std::unique_ptr<ErrorProfile> eprofile = determine_error_profile(args, &err);  // main.rs:27
  if (!eprofile) return die(err);
  // main.rs:30-33
  if (args.error_profile == ErrorProfileKind::CustomShort && eprofile->is_long_read())
    return die("You specified a custom short-read error profile but the provided error profile is for long reads");
  if (args.error_profile == ErrorProfileKind::CustomLong && !eprofile->is_long_read())
    return die("You specified a custom long-read error profile but the provided error profile is for short reads");

  // one engine per entry of --devices (an ordinal may repeat: two engines on one device), or the one of --device
  const std::vector<int> ordinals = args.devices.empty() ? std::vector<int>{args.device} : args.devices;
  if (ordinals.size() > 1 && args.host_fastq) return die("--devices writes the text on the devices: it does not combine with --host-fastq");
  Engines engines;
  side.bam_sort = &engines.bam_sort;
  const std::vector<simmr_engine*>& engs = engines.v;
  for (int ord : ordinals) {
    simmr_engine* en = nullptr;
    if (simmr_engine_create(ord, &en) != SIMMR_OK) return die(std::string("cannot create engine: ") + simmr_last_error(nullptr));
    engines.v.push_back(en);
    // 16-byte read slots wherever the emit kernel of a plan writes them (include/simmr_hip.h: simmr_reads_out); the columns
    // only exist on the --host-fastq path (the text path writes no columns), and DeviceOut::to_host reads either layout
    if (simmr_engine_set_read_slots(en, SIMMR_SLOT16) != SIMMR_OK) return die(simmr_last_error(en));
  }
  simmr_engine* const eng = engs[0];

  info("Loading genomes");
  // main.rs:38-117: the records of --genome-file, or one per --genome
  std::vector<GenomeRecord> records;
  if (args.genome_file) {
    if (!parse_genome_file(*args.genome_file, &records, &err)) return die("Failed to read genome file: " + err);
    for (const auto& rec : records)
      if (!exists(rec.filepath)) return die("Genome (" + rec.filepath + ") does not exist");
  } else {
    for (const auto& path : args.genome) { GenomeRecord r; r.filepath = path; records.push_back(r); }
  }
  std::vector<Genome> genomes;
  const uint64_t min_size = eprofile->minimum_genome_size();
  for (const auto& rec : records) {
    Genome g;
    int rc = 0;  // 1: no usable sequence, the genome is left out
    if (args.host_normalize) {
      if (!Genome::from_fasta(rec.filepath, args.contiguous, &g, &err)) rc = -1;
    } else {  // the sequences normalised, filtered (main.rs:117-162) and packed on the device
      rc = load_genome_device(eng, (uint32_t)genomes.size(), rec.filepath, args.contiguous, min_size, &g, &err);
    }
    if (rc < 0) return die("Failed to parse " + rec.filepath + ": " + err);
    if (rec.uuid) g.uuid = *rec.uuid;
    if (args.genome_file && args.abundance_profile == AbundanceProfileKind::Custom && !rec.abundance)
      return die("You used a custom abundance profile but didn't provide abundances for genome " + g.filepath);
    g.abundance = rec.abundance;
    // every further engine stages its own copy of the reference (replicated, as across ranks: DESIGN.md section 5)
    for (size_t k = 1; !args.host_normalize && rc == 0 && k < engs.size(); k++) {
      Genome again;
      if (load_genome_device(engs[k], (uint32_t)genomes.size(), rec.filepath, args.contiguous, min_size, &again, &err) != 0)
        return die("Failed to stage " + rec.filepath + " on device " + std::to_string(ordinals[k]) + ": " + err);
    }
    if (rc == 0) genomes.push_back(std::move(g));
  }
  if (args.abundance_profile == AbundanceProfileKind::Custom && !args.genome_file)
    return die("a custom abundance profile needs a --genome-file with abundances");

  info("Ensuring genomes meet minimum sequence length requirements for simulation");
  if (!args.contiguous && args.host_normalize) {  // main.rs:117-162
    std::vector<Genome> kept;
    for (Genome& g : genomes) {
      std::vector<Seq> seqs;
      for (Seq& s : g.sequence) {
        if (s.size <= min_size)
          warn("(" + g.filepath + ") Sequence " + s.id + " doesn't meet size requirements, size = " +
               std::to_string(s.size) + ", min size = " + std::to_string(min_size));
        else
          seqs.push_back(std::move(s));
      }
      g.sequence = std::move(seqs);
      if (g.sequence.empty()) { warn("Removing " + g.filepath + " from simulation, it doesn't have usable sequences"); continue; }
      g.num_seqs = g.sequence.size();
      kept.push_back(std::move(g));
    }
    genomes = std::move(kept);
  }
  if (genomes.empty()) return die("no usable genomes");

  std::optional<std::vector<double>> custom_ab;
  if (args.abundance_profile == AbundanceProfileKind::Custom) {
    custom_ab.emplace();
    for (const Genome& g : genomes) custom_ab->push_back(*g.abundance);
  }
  std::unique_ptr<AbundanceProfile> aprofile = determine_abundance_profile(args, custom_ab);

  // ---- stage the references once (replaces keeping Vec<Seq> in RAM for the loop)
  for (size_t gi = 0; args.host_normalize && gi < genomes.size(); gi++) {
    const Genome& g = genomes[gi];
    std::vector<const uint8_t*> ptrs;
    std::vector<uint64_t> lens, sizes;
    for (const Seq& s : g.sequence) { ptrs.push_back((const uint8_t*)s.seq.data()); lens.push_back(s.seq.size()); sizes.push_back(s.size); }
    for (simmr_engine* en : engs)
      if (simmr_stage_genome(en, (uint32_t)gi, (uint32_t)ptrs.size(), ptrs.data(), lens.data(), sizes.data()) != SIMMR_OK)
        return die(std::string("staging failed: ") + simmr_last_error(en));
  }

  // abundances (simulate.rs:121-132 / :334-343)
  const bool is_long = eprofile->is_long_read();
  side.run_paired = !is_long;
  Abundances ab = aprofile->determine_abundances(args.num_reads, genomes.size());
  if (aprofile->is_size_aware()) ab = aprofile->adjust_for_size(genomes, ab, is_long ? 20000 : args.read_length, !is_long);

  // main.rs:191-198: remove previous outputs
  if (is_regular_file(args.output)) remove(args.output.c_str());  // (a pipe or a device given as the output is written to, not replaced)
  const std::string meta_path = args.output + ".tsv";
  if (exists(meta_path)) remove(meta_path.c_str());
  // Once, before the run's first range: --with-ani diverges the staged genomes with the run's seed — that of --seed, or the
  // one the run's first probe_scope drew — and then the side outputs begin (depth[] is laid out for the genomes as they
  // are from now on).
  bool begun = false;
  auto begin_run = [&](const Scope& sc) {
    if (begun) return 0;
    begun = true;
    if (args.with_ani && !diverge_genomes(engs, args, genomes, sc.seed, &side.sites, &side.site_genome, &err)) return die("--with-ani: " + err);
    return side.begin(eng, genomes) ? 0 : die(side.err);
  };

  simmr_error_profile pod = eprofile->pod();
  if (args.rng_philox) {  // (extension) the counter mode, for the profiles that draw per base from a parametric law
    // (a custom model draws base by base only in the k-mer splice of its long-read path: include/simmr_hip.h)
    if (pod.kind == SIMMR_CUSTOM && !is_long)
      return die("--rng philox is not defined for custom-short: its qualities are not drawn base by base and it edits no bases");
    if (pod.kind != SIMMR_PERFECT_SHORT) pod.rng_mode = SIMMR_RNG_PHILOX;  // (perfect-short draws nothing per base)
    if (args.rng_philox_full) {  // the plan from counters too (the library says which profiles it serves)
      if (pod.kind == SIMMR_PERFECT_SHORT || pod.kind == SIMMR_CUSTOM)
        return die("--rng philox-full covers minimal-short, minimal-long and perfect-long");
      pod.rng_mode = SIMMR_RNG_PHILOX_FULL;
    }
  }

  // a unit's FASTQ text, generously: a pair's two records with their headers; a long read is up to 65 535 bases (u16
  // lengths) and the gamma profiles average 20 000 (minimal_long.rs:64-65)
  const uint64_t text_per_unit = is_long ? 2 * 24000 + 260 : 2 * (2 * (uint64_t)args.read_length + 4 + 160);
  const uint64_t chunk_units = args.device_chunk_reads ? std::max<uint64_t>(args.device_chunk_reads / (is_long ? 1 : 2), 1) : auto_chunk_units(text_per_unit);
  // the scope of genomes [g0, g1), with the seed of --seed if there is one
  auto scope = [&](Scope::Kind kind, size_t g0, size_t g1, uint32_t id_base) {
    Scope sc{kind, {}, {}, pod, args.seed ? 1 : 0, args.seed.value_or(0), id_base, text_per_unit};
    for (size_t gi = g0; gi < g1; gi++) { sc.idx.push_back((uint32_t)gi); sc.reads.push_back(ab[gi].first); }
    return sc;
  };
  auto run = [&](const Scope& sc) {
    return engs.size() > 1 ? run_scope_devices(engs, ordinals, args, genomes, sc, chunk_units) : run_scope(eng, args, genomes, sc, chunk_units, &side);
  };
  if (!is_long) {
    info("Simulating short reads");
    // all genomes in one device plan (simulate_pe_reads, simulate.rs:110-150); the library leaves
    // custom profiles to the genome-by-genome loop below
    Scope all = scope(Scope::PE_ALL, 0, genomes.size(), 0);
    const int mrc = probe_scope(eng, &all);
    if (mrc != SIMMR_OK && mrc != SIMMR_ENOTSUP) return die(simmr_last_error(eng));
    if (mrc == SIMMR_OK) {
      if (int rc = begin_run(all)) return rc;
      if (int rc = run(all)) return rc;
    }
    uint32_t id_base = 0;  // the global AtomicU32 of simulate.rs:85-89
    for (size_t gi = 0; mrc == SIMMR_ENOTSUP && gi < genomes.size(); gi++) {
      // the reference draws a fresh entropy seed per genome when there is no --seed (simulate.rs:174)
      Scope sc = scope(Scope::PE_GENOME, gi, gi + 1, id_base);
      if (!sc.has_seed && probe_scope(eng, &sc) != SIMMR_OK) return die(simmr_last_error(eng));
      if (int rc = begin_run(sc)) return rc;
      if (int rc = run(sc)) return rc;
      id_base += (uint32_t)sc.units(0);
    }
  } else {
    info("Simulating long reads");
    Scope sc = scope(Scope::LONG, 0, genomes.size(), 0);
    if (!sc.has_seed && probe_scope(eng, &sc) != SIMMR_OK) return die(simmr_last_error(eng));
    if (int rc = begin_run(sc)) return rc;
    if (int rc = run(sc)) return rc;
  }
  info("Writing simulated reads to " + args.output);
  if (!side.finish(eng, genomes)) return die(side.err);

  // main.rs:213-258
  std::vector<MetadataRow> rows;
  for (size_t gi = 0; gi < genomes.size(); gi++) rows.push_back({genomes[gi].uuid, genomes[gi].filepath, ab[gi].first, ab[gi].second});
  info("Writing simulation metadata to " + meta_path);
  if (!write_metadata(rows, meta_path, &err)) fprintf(stderr, "ERROR simmr-hip: Failed to write metadata file: %s\n", err.c_str());
  return 0;
}

int main(int argc, char** argv) { return run_main(argc, argv); }
