// Stand-alone driver of the planner's deep-lookahead order (csrc/flowplan.cpp window_order), built
// with the host sanitizers by tests/test_flow_window.py: no HIP, no Python in the process.
//   flow_window_driver CASES
// CASES holds one case per line: M N b dtype seglen world rank full nxc tcol steps [NAME=VALUE ...]
// (the fields of tqr_flow_list_spec, the step cap (0: none), then the environment of that case
// alone). Per case the list is built twice, as the environment says and with TQR_DEPTH=0, and the
// driver prints "<tasks> <topological> <permutation of the depth-0 list> <hash> <depth-0 hash>".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <tuple>
#include <vector>

#include "flowplan.hpp"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  if (!in) return 2;
  std::string line;
  std::vector<std::string> set;  // the previous case's variables
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    std::istringstream ls(line);
    tqr_flow_list_spec sp;
    int steps = 0;
    if (!(ls >> sp.M >> sp.N >> sp.b >> sp.dtype >> sp.seglen >> sp.world >> sp.rank >> sp.full >> sp.nxc >> sp.tcol >> steps)) return 2;
    for (const std::string& name : set) unsetenv(name.c_str());
    set.clear();
    std::string depth;  // the case's own TQR_DEPTH, if any
    for (std::string kv; ls >> kv;) {
      const size_t eq = kv.find('=');
      if (eq == std::string::npos) return 2;
      set.push_back(kv.substr(0, eq));
      setenv(set.back().c_str(), kv.c_str() + eq + 1, 1);
      if (set.back() == "TQR_DEPTH") depth = kv.substr(eq + 1);
    }
    tqr::FlowPlan fp, fp0;
    if (tqr::flow_list(sp, fp, steps) != TQR_OK) return 3;
    setenv("TQR_DEPTH", "0", 1);
    const int st0 = tqr::flow_list(sp, fp0, steps);
    if (depth.empty()) unsetenv("TQR_DEPTH");
    else setenv("TQR_DEPTH", depth.c_str(), 1);
    if (st0 != TQR_OK) return 3;
    const int sh = tqr::flow_shape(sp.dtype, sp.b);
    const bool topo = tqr::flow_list_topological(fp.items, sp.M, sp.N, tqr::shape_ns(sh, sp.b));
    auto keys = [](const std::vector<tqr::Item>& L) {
      std::vector<std::tuple<int, int, int, int>> k;
      for (const tqr::Item& it : L) k.emplace_back(it.ts, it.l, it.m, it.k);
      std::sort(k.begin(), k.end());
      return k;
    };
    printf("%zu %d %d %u %u\n", fp.items.size(), (int)topo, (int)(keys(fp.items) == keys(fp0.items)),
           tqr::flow_list_hash(fp.items), tqr::flow_list_hash(fp0.items));
  }
  return 0;
}
