// front_plan_check.cpp -- runs plan_front (csrc/front_plan.cpp) over the golden case list in a stand-alone
// program, for a host build with -fsanitize=address,undefined.  No GPU: plan_front makes no HIP runtime call.
//
//   python tools/front_plan_golden.py --check --cases-text cases.txt
//   C=ookiedokie_amd/csrc
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/front_plan_check.cpp $C/front_plan.cpp $C/loaders.cpp $C/formatter.cpp $C/kernels.hip $C/fir_mfma.hip \
//       $C/fir_tuned.hip -o front_plan_check
//   ./front_plan_check cases.txt
//
// Prints, per run, the number of cases planned and one FNV-1a digest over every result; a sanitizer report is the
// failure.  Case lines: tools/front_plan_golden.py (cases_text).
#include <cinttypes>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>

#include "../ookiedokie_amd/csrc/front_plan.hpp"

using namespace ookd;

namespace {

float f32(const std::string &hex) {
    const uint32_t b = (uint32_t)std::stoul(hex, nullptr, 16);
    float f;
    memcpy(&f, &b, 4);
    return f;
}

double f64(const std::string &hex) {
    const uint64_t b = std::stoull(hex, nullptr, 16);
    double d;
    memcpy(&d, &b, 8);
    return d;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) {
        std::cerr << "usage: front_plan_check CASES.txt\n";
        return 2;
    }
    std::ifstream in(argv[1]);
    std::string line;
    uint64_t all = kFnvBasis;
    unsigned ncases = 0, records = 0;
    while (std::getline(in, line)) {
        std::istringstream w(line);
        std::string thr, nu, a, b;
        uint32_t flags = 0, K = 0, S = 0;
        w >> flags >> thr >> nu >> K;
        std::vector<ookd_rx_carrier> car(K);
        for (auto &c : car) {
            w >> a >> b;
            c = ookd_rx_carrier{};
            c.nu = f64(a);
            c.threshold = f32(b);
        }
        w >> S;
        ookd_filter filt;
        for (uint32_t s = 0; s < S; ++s) {
            FilterStage st;
            uint32_t ntaps = 0;
            w >> st.decimation >> ntaps;
            for (uint32_t k = 0; k < ntaps; ++k) {
                w >> a;
                st.taps.push_back(f32(a));
            }
            filt.total_decimation *= st.decimation;
            filt.stages.push_back(std::move(st));
        }
        if (!w) {
            std::cerr << "bad case line " << ncases + 1 << "\n";
            return 2;
        }
        ookd_front_plan_digest_out d;
        if (ookd_front_plan_digest(flags, f32(thr), S ? &filt : nullptr, f64(nu), car.data(), K, &d) != OOKD_OK) {
            std::cerr << "case " << ncases + 1 << " refused\n";
            return 1;
        }
        all = fnv1a(all, &d, sizeof(d));
        records += d.num_records;
        ++ncases;
    }
    printf("front_plan_check: %u cases, %u carrier records, digest %016" PRIx64 "\n", ncases, records, all);
    return ncases ? 0 : 1;
}
