// stereo_plan_driver.cpp — runs the arithmetic of em-spec_amd/csrc/emspec_stereo_plan.h without a GPU: the per-cell law of the
// stereo image on an array of dB values, exactly as the compose kernel and the host twin call it (stereo_compose_host), and the
// integer palette builder on the colour map of emspec_tables.h.  Every buffer is a heap block of exactly the size the
// definition needs, so that an index past it is ASan's to report.
//   g++ -std=c++17 -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I em-spec_amd/csrc \
//       tests/cdriver/stereo_plan_driver.cpp -o stereo_plan_driver
// tests/test_stereo_cpu.py checks the output.
//   stereo_plan_driver compose IN OUT pairs views a b cells db_top db_range gate_db shift_db pan_range_db
//       IN: float32 [pairs * views][cells]; OUT: level float32 [pairs][cells], index, pan bytes [pairs][cells], rgba
//       [pairs][cells][4] under the palette of brightness 0.5, one after the other.  The map's numbers are given as the
//       hexadecimal of their float32 bits.
//   stereo_plan_driver palette OUT brightness-bits      OUT: [33][256][4]
//   stereo_plan_driver check views a b db_top db_range gate_db shift_db pan_range_db     prints the rule broken, or "ok"
//   stereo_plan_driver abi       prints sizeof(emspec_stereo_map), EMSPEC_ABI_VERSION and the header's pan constants
#include "emspec_stereo_plan.h"
#include "emspec_tables.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace emspec;

static float bits(const char* s) {
    const uint32_t u = (uint32_t)strtoul(s, nullptr, 16);
    float f;
    memcpy(&f, &u, 4);
    return f;
}

static bool write_all(const char* path, const std::vector<std::vector<uint8_t>>& parts) {
    FILE* f = fopen(path, "wb");
    if (!f) return false;
    bool ok = true;
    for (const auto& p : parts) ok = ok && (p.empty() || fwrite(p.data(), 1, p.size(), f) == p.size());
    return fclose(f) == 0 && ok;
}

int main(int argc, char** argv) {
    const std::string op = argc > 1 ? argv[1] : "";
    if (op == "palette" && argc == 4) {
        std::vector<uint8_t> base(1024), pal(kStereoPaletteBytes);
        make_colormap(bits(argv[3]), base.data());
        stereo_palette(base.data(), pal.data());
        return write_all(argv[2], {pal}) ? 0 : 2;
    }
    if (op == "abi") {
        static_assert(EMSPEC_STEREO_PAN_CENTRE == kStereoPanCentre && EMSPEC_STEREO_PAN_LEVELS == kStereoPanLevels, "the header's constants are the plan's");
        printf("%zu %d %d %d\n", sizeof(emspec_stereo_map), EMSPEC_ABI_VERSION, EMSPEC_STEREO_PAN_CENTRE, EMSPEC_STEREO_PAN_LEVELS);
        return 0;
    }
    if (op == "check" && argc == 10) {
        const char* why = stereo_pair_error(atoll(argv[2]), atoll(argv[3]), atoll(argv[4]));
        if (!why) why = stereo_map_error(bits(argv[5]), bits(argv[6]), bits(argv[7]), bits(argv[8]), bits(argv[9]));
        printf("%s\n", why ? why : "ok");
        return 0;
    }
    if (op == "compose" && argc == 14) {
        const long long pairs = atoll(argv[4]), cells = atoll(argv[8]);
        const int views = atoi(argv[5]), a = atoi(argv[6]), b = atoi(argv[7]);
        if (pairs < 0 || cells < 0 || stereo_pair_error(views, a, b)) return 2;
        if (stereo_map_error(bits(argv[9]), bits(argv[10]), bits(argv[11]), bits(argv[12]), bits(argv[13]))) return 2;
        const StereoLaw w = stereo_law(bits(argv[9]), bits(argv[10]), bits(argv[11]), bits(argv[12]), bits(argv[13]));
        const size_t in_n = (size_t)pairs * views * cells, out_n = (size_t)pairs * cells;
        std::vector<float> db(in_n);
        FILE* f = fopen(argv[2], "rb");
        if (!f) return 2;
        const size_t got = in_n ? fread(db.data(), 4, in_n, f) : 0;
        fclose(f);
        if (got != in_n) { fprintf(stderr, "short input\n"); return 2; }
        std::vector<uint8_t> base(1024), pal(kStereoPaletteBytes);
        make_colormap(0.5f, base.data());
        stereo_palette(base.data(), pal.data());
        std::vector<uint8_t> level(out_n * 4), index(out_n), pan(out_n), rgba(out_n * 4);
        stereo_compose_host(db.data(), pairs, views, a, b, cells, w, pal.data(), reinterpret_cast<float*>(level.data()), index.data(),
                            pan.data(), rgba.data());
        return write_all(argv[3], {level, index, pan, rgba}) ? 0 : 2;
    }
    fprintf(stderr, "usage: see the head of stereo_plan_driver.cpp\n");
    return 2;
}
