// eval_cli.hpp — the commands of simmr-hip that run no simulation and score a tool's file against a truth file (eval_cli.cpp), and
// the file walker they and --fit-from-sam go over.  Each answers the process's exit status.
#pragma once
#include <functional>
#include <string>

#include "simmr_host.hpp"

// A file to the device in pieces cut by `rule` (PieceReader; no piece passes what one add takes: SIMMR_ASMEVAL_MAX_BYTES under
// PieceCut::Fasta, SIMMR_FIT_SAM_MAX_BYTES otherwise): add(device, host, n) gets every piece as n bytes of device memory and the
// same n bytes on the host, and answers only when the device has read them (both buffers are then free for the next piece); an
// answer other than 0 ends the walk with that answer.  `flag` names the file's option in the messages.
int file_pieces(const std::string& flag, const std::string& path, simmr_host::PieceCut rule, const std::function<int(const uint8_t*, const char*, size_t)>& add);
// 0 where the file of option `flag` opens for reading; the message and 1 where not.
int probe_file(const std::string& flag, const std::string& path);

int run_eval_sam(const simmr_host::CliArgs& args);
int run_eval_overlaps(const simmr_host::CliArgs& args);
int run_eval_vcf(const simmr_host::CliArgs& args);
int run_eval_classified(const simmr_host::CliArgs& args);
int run_eval_assembly(const simmr_host::CliArgs& args);
int run_eval_placement(const simmr_host::CliArgs& args);
int run_eval_bins(const simmr_host::CliArgs& args);
int run_eval_corrected(const simmr_host::CliArgs& args);
