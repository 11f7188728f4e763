// Walks csrc/dcx_lm_dev.h's Levenberg-Marquardt automaton on the host: no HIP, no GPU (tests/test_lm_host.py compiles and runs it).
// usage: lm_host NG STOP_FORCED        NG = 6 or 9, STOP_FORCED = 0 or 1
// stdin: "init_cost units points", then one attempt per line: "cost dn pn bad" (inf and nan are read as such).  The global
// parameters stay zero, so they add nothing to dn and pn.
// stdout: after the init and after every attempt one line
//   code lg iters attempts verdict status prev_cost rms result_iters result_attempts
// (status, rms and the two counts as the result words hold them).  Nothing is read once the state word says finished.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../deepcharuco_amd/csrc/dcx_lm_dev.h"

template <int NG, bool STOP_FORCED>
static int run() {
    LmState<NG> st;
    std::memset(&st, 0, sizeof(st));
    lm_reset(&st);
    st.code = kNextEvaluate;
    char c[64], d[64], p[64];
    int bad = 0;
    if (std::scanf("%63s %63s %63s", c, d, p) != 3) return 2;
    const double units = std::strtod(d, nullptr), points = std::strtod(p, nullptr);
    bool init = true;
    double cost = std::strtod(c, nullptr), dn = 0.0, pn = 0.0;
    for (;;) {
        const int verdict = lm_decide<NG, STOP_FORCED>(&st, init, cost, dn, pn, units, points, bad != 0);
        std::printf("%d %d %d %d %d %d %.17g %.17g %d %d\n", st.code, st.lg, st.iters, st.attempts, verdict, (int)st.result[NG + 5],
                    st.prev_cost, st.result[NG], (int)st.result[NG + 1], (int)st.result[NG + 2]);
        init = false;
        if (st.code == kFinished || std::scanf("%63s %63s %63s %d", c, d, p, &bad) != 4) return 0;
        cost = std::strtod(c, nullptr);
        dn = std::strtod(d, nullptr);
        pn = std::strtod(p, nullptr);
    }
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const int ng = std::atoi(argv[1]), stop = std::atoi(argv[2]);
    if (ng == 6) return stop ? run<6, true>() : run<6, false>();
    if (ng == 9) return stop ? run<9, true>() : run<9, false>();
    return 2;
}
