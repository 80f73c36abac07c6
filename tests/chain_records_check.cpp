// chain_records_check.cpp — prints the node tree and the chain records that smplsim_amd/csrc/ss_tables.h builds for the body trees
// given on the command line (one argument per tree: the parents of its bodies, comma-separated, -1 for the root), one line per
// tree: nlev | ndepth | chainnode | the records as 32-bit words.  Built and read by tests/test_chain_records_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../smplsim_amd/csrc/ss_tables.h"

int main(int argc, char **argv) {
  for (int a = 1; a < argc; a++) {
    ss::Tree t;
    for (char *tok = std::strtok(argv[a], ","); tok; tok = std::strtok(nullptr, ",")) t.parent.push_back(std::atoi(tok));
    if (const char *e = ss::node_tree(t)) { std::printf("error %s\n", e); continue; }
    ss::chain_records(t);
    std::printf("%d |", t.nlev);
    for (int v : t.ndepth) std::printf(" %d", v);
    std::printf(" |");
    for (int v : t.chainnode) std::printf(" %d", v);
    std::printf(" |");
    for (uint32_t v : t.chainrec) std::printf(" %u", v);
    std::printf("\n");
  }
  return 0;
}
