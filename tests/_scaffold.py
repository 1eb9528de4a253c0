"""What the guards of the scorer units ask of simmr_amd/csrc/scorer_host.hpp, the host scaffold they share."""
import re
from pathlib import Path

CSRC = Path(__file__).resolve().parent.parent / "simmr_amd" / "csrc"


def sorts_through_the_pair_sort(unit):
    """the unit sorts with the shared sort and defines none of its own: it owns a PairSort and calls its sort, and PairSort::sort
    is the scaffold's one call of sam_sort.hip's samsort_sort_pairs"""
    text, scaffold = (CSRC / unit).read_text(), (CSRC / "scorer_host.hpp").read_text()
    sort = re.search(r"struct PairSort \{.*?\n\};", scaffold, re.S)
    return bool('#include "scorer_host.hpp"' in text and re.search(r"^  PairSort \w+", text, re.M) and re.search(r"\bsort\(st, ", text)
                and sort and sort.group(0).count("samsort_sort_pairs(") == 1 and scaffold.count("samsort_sort_pairs(") == 1
                and "__global__" not in text and "__global__" not in scaffold)
