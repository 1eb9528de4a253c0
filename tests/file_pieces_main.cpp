// file_pieces_main.cpp — PieceReader and piece_cut of simmr_amd/host/host.cpp in a stand-alone program, for a build under the
// sanitizers (tests/test_file_pieces_host.py).
//   file_pieces_main PATH RULE PIECE LIMIT     RULE: newline, fasta, or record:K for records of K lines; PIECE: the bytes of one
//                                              read; LIMIT: the most bytes a piece may have
// Prints, per piece, a line "piece N", the piece's N bytes and a newline; then a line "end NAME AT" with NAME one of done,
// cannot-read, too-long and AT the bytes of the file consumed when the walk ended (-1 where the file does not say).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../simmr_amd/host/simmr_host.hpp"

using namespace simmr_host;

int main(int argc, char** argv) {
  if (argc != 5) { fprintf(stderr, "usage: file_pieces_main PATH RULE PIECE LIMIT\n"); return 2; }
  const std::string rule_name = argv[2];
  PieceCut rule;
  if (rule_name == "newline") rule.kind = PieceCut::Newline;
  else if (rule_name == "fasta") rule.kind = PieceCut::Fasta;
  else if (rule_name.rfind("record:", 0) == 0) { rule.kind = PieceCut::Record; rule.lines = (uint32_t)strtoul(rule_name.c_str() + 7, nullptr, 10); }
  else { fprintf(stderr, "unknown rule %s\n", argv[2]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  PieceReader reader(f, rule, strtoull(argv[4], nullptr, 10), strtoull(argv[3], nullptr, 10));
  const uint8_t* p = nullptr;
  size_t n = 0;
  PieceReader::End end;
  while ((end = reader.next(&p, &n)) == PieceReader::Piece) {
    printf("piece %zu\n", n);
    fwrite(p, 1, n, stdout);
    putchar('\n');
  }
  printf("end %s %ld\n", end == PieceReader::Done ? "done" : end == PieceReader::CannotRead ? "cannot-read" : "too-long", ftell(f));
  fclose(f);
  return 0;
}
