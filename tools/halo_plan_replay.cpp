// tools/halo_plan_replay.cpp -- pcl::OverlapPlan (pyclaw_amd/csrc/halo_plan.hpp) driven from a script on standard input,
// without the library and without a device: one event per line, "event a b" as pcl_halo_plan_trace takes them
// (include/pyclaw_amd.h); the answers go to standard output, one per line.  For runs of the header under the host
// sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o halo_plan_replay tools/halo_plan_replay.cpp
#include <cstdio>
#include <vector>

#include "../pyclaw_amd/csrc/halo_plan.hpp"

int main() {
    std::vector<int> event, a, b;
    int e, x, y;
    while (scanf("%d %d %d", &e, &x, &y) == 3) {
        event.push_back(e);
        a.push_back(x);
        b.push_back(y);
    }
    std::vector<int> out(event.size(), -99);
    if (const char *bad = pcl::overlap_plan_trace((long)event.size(), event.data(), a.data(), b.data(), out.data())) {
        fprintf(stderr, "%s\n", bad);
        return 1;
    }
    for (int o : out) printf("%d\n", o);
    return 0;
}
