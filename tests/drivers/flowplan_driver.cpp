// Stand-alone driver of the task-list planner (csrc/flowplan.cpp), built with the host sanitizers
// by tests/test_flowplan.py: no HIP, no Python in the process.
//   flowplan_driver CASES
// CASES holds one case per line: M N b dtype seglen world rank full nxc tcol [NAME=VALUE ...]
// (the fields of tqr_flow_list_spec, then the environment of that case alone). Per case it prints
// "<tasks> <est_order> <FNV-1a hash of the list>", or "EINVAL"; at the end "missed <n>", the
// dependency lookups of the estimator's key bump that found no task, summed over all cases.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "flowplan.hpp"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  if (!in) return 2;
  std::string line;
  std::vector<std::string> set;  // the previous case's variables
  long missed = 0;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    std::istringstream ls(line);
    tqr_flow_list_spec sp;
    if (!(ls >> sp.M >> sp.N >> sp.b >> sp.dtype >> sp.seglen >> sp.world >> sp.rank >> sp.full >> sp.nxc >> sp.tcol)) return 2;
    for (const std::string& name : set) unsetenv(name.c_str());
    set.clear();
    for (std::string kv; ls >> kv;) {
      const size_t eq = kv.find('=');
      if (eq == std::string::npos) return 2;
      set.push_back(kv.substr(0, eq));
      setenv(set.back().c_str(), kv.c_str() + eq + 1, 1);
    }
    tqr::FlowPlan fp;
    if (tqr::flow_list(sp, fp) != TQR_OK) {
      printf("EINVAL\n");
      continue;
    }
    missed += fp.missed;
    printf("%zu %d %u\n", fp.items.size(), (int)fp.est_order, tqr::flow_list_hash(fp.items));
  }
  printf("missed %ld\n", missed);
  return 0;
}
