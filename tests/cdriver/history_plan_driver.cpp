// history_plan_driver.cpp — runs the arithmetic of em-spec_amd/csrc/emspec_history_plan.h without a GPU, on one stream: in
// place of live_history_store_kernel a model of what its workgroups do to the ring (one per column of a launch, in any order:
// which columns are stored, in which slot, and how often a slot is written in one launch), and in place of history_view_kernel
// the columns a view's groups read - once through the slot runs (history_runs) and once the kernel's way, the first slot from
// history_group_slot and then one compare per column (history_next_slot).  The ring is a host block of exactly W entries, each
// carrying the column that wrote it, so that a wrong slot is ASan's to report.
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I em-spec_amd/csrc \
//       tests/cdriver/history_plan_driver.cpp -o history_plan_driver
// tests/test_history_plan_cpu.py checks the output.  Input, one line each:
//   ring W | launch COUNT | reset | view FIRST F GROUPS | bytes S W ROWS
// Output: a JSON list, one object per line.
#include "emspec_history_plan.h"

#include <algorithm>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

using namespace emspec;

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: see the head of history_plan_driver.cpp\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::string line;
    int64_t W = 0, end = 0;
    std::vector<long long> ring;   // [W]: the column each slot holds, -1: none
    bool first = true;
    printf("[");
    while (std::getline(in, line)) {
        std::istringstream w(line);
        std::string op;
        if (!(w >> op)) continue;
        long long a = 0, b = 0, c = 0;
        w >> a >> b >> c;
        printf("%s{\"op\":\"%s\"", first ? "" : ",\n", op.c_str());
        first = false;
        if (op == "ring") {
            W = a; end = 0;
            ring.assign((size_t)W, -1);
            ring.shrink_to_fit();
        } else if (op == "reset") {
            end = 0;
            ring.assign((size_t)W, -1);
        } else if (op == "launch") {
            // the stream emits columns [end, end + COUNT): one workgroup per column, last to first (any order must do)
            const int64_t c0 = end, count = a;
            std::vector<int> writes((size_t)W, 0);
            int most = 0;
            printf(",\"stored\":[");
            bool f1 = true;
            for (int64_t col = c0 + count - 1; col >= c0; --col) {
                if (!history_stores(col, c0, count, W)) continue;
                const int64_t slot = history_slot(col, W);
                ring.at((size_t)slot) = col;
                most = std::max(most, ++writes.at((size_t)slot));
                printf("%s%lld", f1 ? "" : ",", (long long)col);
                f1 = false;
            }
            end = c0 + count;
            printf("],\"most_writes\":%d,\"keep_from\":%lld", most, (long long)history_keep_from(c0, count, W));
        } else if (op == "view") {
            const int64_t vfirst = a, f = b, groups = c;
            const int rc = history_view_check(vfirst, f, groups, end, W);
            printf(",\"rc\":%d,\"groups\":[", rc);
            for (int64_t g = 0; rc == kHistoryViewOk && g < groups; ++g) {
                const HistoryGroup grp = history_group(vfirst, f, g, end);
                const HistoryRuns r = history_runs(grp.c0, grp.c1 - grp.c0, W);
                printf("%s{\"c\":[%lld,%lld],\"runs\":[%lld,%lld,%lld],\"by_runs\":[", g ? "," : "", (long long)grp.c0, (long long)grp.c1,
                       (long long)r.slot0, (long long)r.n0, (long long)r.n1);
                for (int64_t k = 0; k < r.n0; ++k) printf("%s%lld", k ? "," : "", ring.at((size_t)(r.slot0 + k)));
                for (int64_t k = 0; k < r.n1; ++k) printf(",%lld", ring.at((size_t)k));
                printf("],\"by_walk\":[");
                int slot = history_group_slot((int)history_slot(vfirst, W), (int)(g * f), (int)W);
                for (int64_t col = grp.c0; col < grp.c1; ++col) {
                    printf("%s%lld", col > grp.c0 ? "," : "", ring.at((size_t)slot));
                    slot = history_next_slot(slot, (int)W);
                }
                printf("]}");
            }
            printf("]");
        } else if (op == "bytes") {
            printf(",\"bytes\":%llu,\"cells\":%llu", (unsigned long long)history_ring_bytes((int)a, b, (int)c),
                   (unsigned long long)history_view_cells((int)a, b, (int)c));
        } else {
            return 2;
        }
        printf(",\"end\":%lld,\"first\":%lld,\"ring\":[", (long long)end, (long long)(W ? history_first(end, W) : 0));
        for (size_t k = 0; k < ring.size(); ++k) printf("%s%lld", k ? "," : "", ring[k]);
        printf("]}");
    }
    printf("]\n");
    return 0;
}
