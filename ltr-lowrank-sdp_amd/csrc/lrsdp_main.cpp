// lrsdp_main.cpp -- drop-in replacement for the LoRADS CLI binary
// (`LoRADS_v_2_0_1-alpha <file.dat-s> --flag value ... --jsonfile out.json`) that
// benchmark.py (benchmark.py:240-262) and dataset/run_lorads.sh call.  Same
// argv contract as src_semi/main.c:256-348 (argv[1] = instance, getopt_long
// flags main.c:125-154, unknown flags ignored, exit code 0), plus the three
// flags the reference never implemented (--rankSchedule, --nearStallFactor,
// --disableOracle) and --device.  The solve runs on the MI355X
// through liblrsdp.so (include/lrsdp.h).
// `--batch FILE` solves many instances in this one process (lrs_solve_batch): each non-empty
// line of FILE is `<instance.dat-s> <jsonfile> [flags...]`, the line's flags parsed by the same
// table on top of the command line's.  Exit code 1 if any instance failed (named on stderr).
// `--roundTrials T` (a multiple of 64; default 0 = off) rounds the solve's R to +-1 assignments
// (lrs_round_signs) when every cone is diagonally constrained: `--roundSeed S`
// (default 0), `--roundLocalSearch 0|1` (default 1), `--roundFile PATH` (the best assignment, one
// +1 / -1 a line in cone order); the JSON gains a "rounding" object.  A problem that does not
// qualify keeps its output as it is, with one line on stderr.
// `--triangleCuts K` (default 0 = off) then finds the K most violated triangle inequalities of
// every diagonally constrained cone's R (lrs_separate_triangles) with violation
// above `--triangleMinViol v` (default 0); `--triangleFile PATH` receives them, `i j k type
// violation` a line (i < j < k 1-based, type 0..3, %.17g); the JSON gains a "triangles" object.  A
// cone that does not qualify gets one line on stderr and nothing else.
// `--compressTol t` (with `--compressSlack s`, default 0) after the last solve rotates the final
// point to the principal axes of its Gram and keeps the eigenvalues above t times the largest, plus
// s (lrs_factor_compress; the source is (U + V) / 2 if the ADMM phase ran, else R);
// the JSON gains a "compressed" object {"ranks", "lost_trace", "spectrum"}.  With --cutRounds the
// loop also compresses R before every warm re-solve.  `--rankShrink t` turns the in-solve hook on
// (lrs_set_rank_shrink(t, s)): the ADMM phase runs at the ranks the ALM point needs.  --batch
// ignores the three.
#include <getopt.h>

#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/lrsdp.h"

extern "C" int lrs_set_log_path(lrs_ctx *ctx, const char *path);

static bool parse_schedule(const char *path, std::vector<int> &out) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    std::string s;
    char buf[4096];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) s.append(buf, n);
    fclose(f);
    size_t k = s.find("\"rank_schedule\"");
    if (k == std::string::npos) return false;
    k = s.find('[', k);
    size_t e = s.find(']', k);
    if (k == std::string::npos || e == std::string::npos) return false;
    const char *p = s.c_str() + k + 1, *end = s.c_str() + e;
    while (p < end) {
        char *q;
        long v = strtol(p, &q, 10);
        if (q == p) { p++; continue; }
        out.push_back((int)v);
        p = q;
    }
    return !out.empty();
}

static std::string problem_name(const char *path) {   // set_problem_name, lorads_logging.c
    std::string s(path);
    size_t sl = s.find_last_of('/');
    if (sl != std::string::npos) s = s.substr(sl + 1);
    size_t dot = s.find('.');
    if (dot != std::string::npos) s = s.substr(0, dot);
    return s;
}

// the flags of one instance: the command line's, then (--batch) its manifest line's on top
struct Flags {
    lrs_params p;
    std::string logFile, jsonFile, schedFile, batchFile;
    int device = 0;
    int roundTrials = 0, roundLocalSearch = 1;
    unsigned long long roundSeed = 0;
    std::string roundFile;
    int triangleCuts = 0;
    double triangleMinViol = 0.0;
    std::string triangleFile;
    int cutRounds = 0;
    bool cutDrop = false;
    double cutDropSlack = 0.0;
    double compressTol = -1.0, rankShrink = 0.0;   // < 0 / <= 0: off
    int compressSlack = 0;
};
static void parse_flags(int argc, char **argv, Flags &F) {
    lrs_params &p = F.p;
    static struct option opts[] = {
        {"logfile", required_argument, 0, 1025}, {"jsonfile", required_argument, 0, 1026},
        {"initRho", required_argument, 0, 1000}, {"rhoMax", required_argument, 0, 1001},
        {"rhoCellingALM", required_argument, 0, 1002}, {"rhoCellingADMM", required_argument, 0, 1003},
        {"maxALMIter", required_argument, 0, 1004}, {"maxADMMIter", required_argument, 0, 1005},
        {"timesLogRank", required_argument, 0, 1006}, {"fixedRank", required_argument, 0, 1022},
        {"initRank", required_argument, 0, 1023}, {"rhoFreq", required_argument, 0, 1007},
        {"rhoFactor", required_argument, 0, 1008}, {"ALMRhoFactor", required_argument, 0, 1009},
        {"rankUpdateFactor", required_argument, 0, 1024}, {"phase1Tol", required_argument, 0, 1010},
        {"phase2Tol", required_argument, 0, 1011}, {"timeSecLimit", required_argument, 0, 1012},
        {"heuristicFactor", required_argument, 0, 1013}, {"lbfgsListLength", required_argument, 0, 1014},
        {"endTauTol", required_argument, 0, 1015}, {"endALMSubTol", required_argument, 0, 1016},
        {"l2Rescaling", required_argument, 0, 1017}, {"reoptLevel", required_argument, 0, 1018},
        {"dyrankLevel", required_argument, 0, 1019}, {"highAccMode", required_argument, 0, 1020},
        {"oracleRankNaive", no_argument, 0, 1021},
        {"rankSchedule", required_argument, 0, 2000}, {"nearStallFactor", required_argument, 0, 2001},
        {"disableOracle", no_argument, 0, 2002}, {"device", required_argument, 0, 2003},
        {"quiet", no_argument, 0, 2004}, {"batch", required_argument, 0, 2005},
        {"roundTrials", required_argument, 0, 2006}, {"roundSeed", required_argument, 0, 2007},
        {"roundLocalSearch", required_argument, 0, 2008}, {"roundFile", required_argument, 0, 2009},
        {"triangleCuts", required_argument, 0, 2010}, {"triangleMinViol", required_argument, 0, 2011},
        {"triangleFile", required_argument, 0, 2012}, {"cutRounds", required_argument, 0, 2013},
        {"cutDropSlack", required_argument, 0, 2014}, {"compressTol", required_argument, 0, 2015},
        {"compressSlack", required_argument, 0, 2016}, {"rankShrink", required_argument, 0, 2017}, {0, 0, 0, 0}};
    int opt, li = 0;
    optind = 0;   // a fresh scan (one per manifest line)
    while ((opt = getopt_long(argc, argv, "r:", opts, &li)) != -1) {
        switch (opt) {
        case 1025: F.logFile = optarg; break;
        case 1026: F.jsonFile = optarg; break;
        case 1000: p.initRho = atof(optarg); break;
        case 1001: p.rhoMax = atof(optarg); break;
        case 1002: p.rhoCellingALM = atof(optarg); break;
        case 1003: p.rhoCellingADMM = atof(optarg); break;
        case 1004: p.maxALMIter = atoi(optarg); break;
        case 1005: p.maxADMMIter = atoi(optarg); break;
        case 1006: p.timesLogRank = atof(optarg); break;
        case 1022: p.fixedRank = atoi(optarg); break;
        case 1023: p.initRank = atoi(optarg); break;
        case 1007: p.rhoFreq = atoi(optarg); break;
        case 1008: p.rhoFactor = atof(optarg); break;
        case 1009: p.ALMRhoFactor = atof(optarg); break;
        case 1024: p.rankUpdateFactor = atof(optarg); break;
        case 1010: p.phase1Tol = atof(optarg); break;
        case 1011: p.phase2Tol = atof(optarg); break;
        case 1012: p.timeSecLimit = atof(optarg); break;
        case 1013: p.heuristicFactor = atof(optarg); break;
        case 1014: p.lbfgsListLength = atoi(optarg); break;
        case 1015: p.endTauTol = atof(optarg); break;
        case 1016: p.endALMSubTol = atof(optarg); break;
        case 1017: p.l2Rescaling = atoi(optarg); break;
        case 1018: p.reoptLevel = atoi(optarg); break;
        case 1019: p.dyrankLevel = atoi(optarg); break;
        case 1020: p.highAccMode = atoi(optarg); break;
        case 1021: p.oracleRankNaive = 1; break;
        case 2000: F.schedFile = optarg; break;
        case 2001: p.nearStallFactor = atof(optarg); break;
        case 2002: p.disableOracle = 1; break;
        case 2003: F.device = atoi(optarg); break;
        case 2004: p.verbose = 0; break;
        case 2005: F.batchFile = optarg; break;
        case 2006: F.roundTrials = atoi(optarg); break;
        case 2007: F.roundSeed = strtoull(optarg, nullptr, 10); break;
        case 2008: F.roundLocalSearch = atoi(optarg); break;
        case 2009: F.roundFile = optarg; break;
        case 2010: F.triangleCuts = atoi(optarg); break;
        case 2011: F.triangleMinViol = atof(optarg); break;
        case 2012: F.triangleFile = optarg; break;
        case 2013: F.cutRounds = atoi(optarg); break;
        case 2014: F.cutDrop = true; F.cutDropSlack = atof(optarg); break;
        case 2015: F.compressTol = atof(optarg); break;
        case 2016: F.compressSlack = atoi(optarg); break;
        case 2017: F.rankShrink = atof(optarg); break;
        default: break;   // unknown flags: getopt already printed a message; ignored like main.c
        }
    }
}
// what follows the scan: the schedule file (sched keeps the array p points to), the L-BFGS floor
static void finish_flags(Flags &F, std::vector<int> &sched) {
    lrs_params &p = F.p;
    if (!F.schedFile.empty()) {
        if (parse_schedule(F.schedFile.c_str(), sched)) {
            p.rankSchedule = sched.data();
            p.rankScheduleLen = (int)sched.size();
        } else {
            fprintf(stderr, "[lrsdp] could not parse rank schedule %s; ignored\n", F.schedFile.c_str());
        }
    }
    if (p.lbfgsListLength < 1) {   // the reference's ring needs one node at least (data/lorads_solver.c:686-706)
        fprintf(stderr, "[lrsdp] lbfgsListLength %d < 1; using 2\n", p.lbfgsListLength);
        p.lbfgsListLength = 2;
    }
}

// lrs_write_json's text ends with the top-level closing brace: `obj` (from its leading comma to the
// new closing brace) takes the place of that brace and the white space before it
static void json_append(const char *jsonFile, const std::string &obj) {
    FILE *f = fopen(jsonFile, "rb");
    if (!f) return;
    std::string s;
    char buf[4096];
    size_t nr;
    while ((nr = fread(buf, 1, sizeof(buf), f)) > 0) s.append(buf, nr);
    fclose(f);
    const size_t close = s.find_last_of('}');
    if (close == std::string::npos) return;
    size_t end = close;
    while (end > 0 && isspace((unsigned char)s[end - 1])) end--;
    s = s.substr(0, end) + obj;
    f = fopen(jsonFile, "wb");
    if (!f) return;
    fwrite(s.data(), 1, s.size(), f);
    fclose(f);
}

// --roundTrials T after a solve: every cone's R rounded on the context's own stream (per cone the
// same seed), the best values summed (cones with only diagonal constraints are independent).  On
// success the JSON at jsonFile (if any) gains "rounding" before its closing brace and roundFile
// receives the assignment; a cone that does not qualify leaves both as they are (one stderr line).
// sdp_only: after cut rounds the last cone is the cuts' LP block, which is not rounded.
static void round_and_report(lrs_ctx *ctx, const Flags &F, const char *jsonFile, bool sdp_only = false) {
    if (F.roundTrials <= 0) return;
    int K = 0;
    lrs_problem_info(ctx, nullptr, &K, nullptr, nullptr, nullptr);
    std::vector<int> dims(K > 0 ? K : 1);
    lrs_problem_info(ctx, nullptr, nullptr, dims.data(), nullptr, nullptr);
    if (sdp_only) K = 1;
    std::vector<signed char> x;
    std::vector<int> best(K, 0);
    double value = 0.0, secs = 0.0;
    int sweeps = 0;
    for (int k = 0; k < K; ++k) {
        std::vector<signed char> xk(dims[k] > 0 ? dims[k] : 1);
        double v = 0.0;
        int sw = 0;
        lrs_sync(ctx);
        timespec t0, t1;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        const int rc = lrs_round_signs(ctx, k, LRS_R, F.roundTrials, nullptr, F.roundSeed, F.roundLocalSearch, 0, nullptr,
                                       nullptr, &best[k], &v, xk.data(), &sw);
        clock_gettime(CLOCK_MONOTONIC, &t1);
        if (rc) {
            fprintf(stderr, "[lrsdp] rounding skipped: %s\n", lrs_last_error());
            return;
        }
        secs += (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
        value += v;
        sweeps = sw > sweeps ? sw : sweeps;
        x.insert(x.end(), xk.begin(), xk.begin() + dims[k]);
    }
    std::string bt = K == 1 ? std::to_string(best[0]) : "[";
    for (int k = 0; K != 1 && k < K; ++k) bt += (k ? ", " : "") + std::to_string(best[k]);
    if (K != 1) bt += "]";
    printf("Rounding: %d trials, seed %llu, local search %d: value %.10e (sweeps %d, %f s)\n", F.roundTrials, F.roundSeed,
           F.roundLocalSearch ? 1 : 0, value, sweeps, secs);
    if (!F.roundFile.empty()) {
        FILE *f = fopen(F.roundFile.c_str(), "w");
        if (!f) fprintf(stderr, "[lrsdp] cannot open %s\n", F.roundFile.c_str());
        else {
            for (signed char s : x) fprintf(f, "%d\n", (int)s);
            fclose(f);
        }
    }
    if (!jsonFile) return;
    char obj[512];
    snprintf(obj, sizeof(obj),
             ",\n  \"rounding\": {\n    \"trials\": %d,\n    \"seed\": %llu,\n    \"local_search\": %d,\n"
             "    \"value\": %.16e,\n    \"best_trial\": %s,\n    \"sweeps\": %d,\n    \"time_sec\": %.16e\n  }\n}\n",
             F.roundTrials, F.roundSeed, F.roundLocalSearch ? 1 : 0, value, bt.c_str(), sweeps, secs);
    json_append(jsonFile, obj);
}

// --triangleCuts K after a solve (and after the rounding): every cone's R separated on the
// context's own stream.  The cones that qualify are reported in cone order: the JSON at jsonFile
// (if any) gains "triangles" (n_cuts, n_violated, max_violation, time_sec: numbers with one such
// cone, lists with several) and triangleFile receives their cuts ("# cone k" before each cone's
// lines when there are several).  A cone that does not qualify costs one stderr line.
static void triangles_and_report(lrs_ctx *ctx, const Flags &F, const char *jsonFile) {
    if (F.triangleCuts <= 0) return;
    int K = 0;
    lrs_problem_info(ctx, nullptr, &K, nullptr, nullptr, nullptr);
    const int cap = F.triangleCuts < LRS_TRI_MAX_K ? F.triangleCuts : LRS_TRI_MAX_K;
    struct Cone {
        int k, n_cuts;
        long long n_violated;
        double max_violation, secs;
        std::vector<int> cuts;
        std::vector<double> viol;
    };
    std::vector<Cone> done;
    for (int k = 0; k < K; ++k) {
        Cone c;
        c.k = k;
        c.cuts.resize(4 * (size_t)cap);
        c.viol.resize(cap);
        lrs_sync(ctx);
        timespec t0, t1;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        const int rc = lrs_separate_triangles(ctx, k, LRS_R, F.triangleCuts, F.triangleMinViol, c.cuts.data(), c.viol.data(),
                                              &c.n_cuts, &c.n_violated, &c.max_violation);
        clock_gettime(CLOCK_MONOTONIC, &t1);
        if (rc) {
            fprintf(stderr, "[lrsdp] triangles skipped: %s\n", lrs_last_error());
            continue;
        }
        c.secs = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
        printf("Triangles: cone %d: %lld violated by more than %g (largest %.10e), %d returned (%f s)\n", k, c.n_violated,
               F.triangleMinViol, c.max_violation, c.n_cuts, c.secs);
        done.push_back(std::move(c));
    }
    if (done.empty()) return;
    if (!F.triangleFile.empty()) {
        FILE *f = fopen(F.triangleFile.c_str(), "w");
        if (!f) fprintf(stderr, "[lrsdp] cannot open %s\n", F.triangleFile.c_str());
        else {
            for (const Cone &c : done) {
                if (done.size() > 1) fprintf(f, "# cone %d\n", c.k + 1);
                for (int t = 0; t < c.n_cuts; ++t)
                    fprintf(f, "%d %d %d %d %.17g\n", c.cuts[4 * t] + 1, c.cuts[4 * t + 1] + 1, c.cuts[4 * t + 2] + 1,
                            c.cuts[4 * t + 3], c.viol[t]);
            }
            fclose(f);
        }
    }
    if (!jsonFile) return;
    auto list = [&](auto field) {
        std::string s = done.size() == 1 ? "" : "[";
        for (size_t q = 0; q < done.size(); ++q) s += (q ? ", " : "") + field(done[q]);
        return done.size() == 1 ? s : s + "]";
    };
    auto num = [](double v) {
        char b[40];
        snprintf(b, sizeof(b), "%.16e", v);
        return std::string(b);
    };
    char head[160];
    snprintf(head, sizeof(head), ",\n  \"triangles\": {\n    \"max_cuts\": %d,\n    \"min_violation\": %.16e,\n",
             F.triangleCuts, F.triangleMinViol);
    const std::string obj = std::string(head) +
        "    \"n_cuts\": " + list([](const Cone &c) { return std::to_string(c.n_cuts); }) + ",\n" +
        "    \"n_violated\": " + list([](const Cone &c) { return std::to_string(c.n_violated); }) + ",\n" +
        "    \"max_violation\": " + list([&](const Cone &c) { return num(c.max_violation); }) + ",\n" +
        "    \"time_sec\": " + list([&](const Cone &c) { return num(c.secs); }) + "\n  }\n}\n";
    json_append(jsonFile, obj);
}

// --cutRounds N (with --triangleCuts K) after the first solve: the cutting-plane loop of DESIGN.md
// §4.14 in the one context.  Round 0 is the solve just done; each later round separates K + E
// inequalities at R (E: registered cuts violated by more than --triangleMinViol), takes the K most
// violated that are not registered, stops when none is new, drops cuts with slack > --cutDropSlack
// and a multiplier >= 0 (if given), appends with carry and re-solves warm.  `r` ends as the last
// solve's result; `rounds` receives the JSON array's text; triangleFile the final cut list as `i j k
// type violation` (1-based, the violation at the final R: minus the cut's slack).  A problem that
// does not qualify keeps the first solve and costs one stderr line.
static void cut_rounds(lrs_ctx *ctx, const Flags &F, lrs_result &r, std::string &rounds) {
    auto now = []() {
        timespec t;
        clock_gettime(CLOCK_MONOTONIC, &t);
        return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
    };
    auto num = [](double v) {
        char b[40];
        snprintf(b, sizeof(b), "%.16e", v);
        return std::string(b);
    };
    const int K = F.triangleCuts < LRS_TRI_MAX_K ? F.triangleCuts : LRS_TRI_MAX_K;
    int ncut = 0;
    auto record = [&](double t0, int added, int dropped, long long nviol, double maxv) -> bool {
        double bound = 0.0, best = 0.0;
        int conv = 0;
        if (lrs_certified_bound(ctx, &bound, nullptr, &conv)) return false;
        if (F.roundTrials > 0 && lrs_round_signs(ctx, 0, LRS_R, F.roundTrials, nullptr, F.roundSeed, F.roundLocalSearch, 0,
                                                 nullptr, nullptr, nullptr, &best, nullptr, nullptr))
            return false;
        lrs_cuts_get(ctx, nullptr, 0, &ncut);
        std::string o = rounds.empty() ? "\n    {" : ",\n    {";
        o += "\"n_cuts\": " + std::to_string(ncut) + ", \"n_added\": " + std::to_string(added) + ", \"n_dropped\": " +
             std::to_string(dropped) + ", \"n_violated\": " + std::to_string(nviol) + ", \"max_violation\": " + num(maxv) +
             ", \"pobj\": " + num(r.pobj) + ", \"dobj\": " + num(r.dobj) + ", \"certified_bound\": " + num(bound) +
             ", \"bound_converged\": " + (conv ? "true" : "false") + ", \"alm_inner\": " + std::to_string(r.alm_inner) +
             ", \"admm_iter\": " + std::to_string(r.admm_iter);
        if (F.roundTrials > 0) o += ", \"best_value\": " + num(best);
        o += ", \"time_sec\": " + num(now() - t0) + "}";
        rounds += o;
        printf("Cut round: %d cuts (+%d -%d), %lld violated (largest %.6e), pObj %.10e, certified bound %.10e%s\n", ncut,
               added, dropped, nviol, maxv, r.pobj, bound, conv ? "" : " (eigen-solve not converged)");
        return true;
    };
    double t0 = now() - r.solve_time;
    long long nviol = 0;
    double maxv = 0.0;
    if (lrs_separate_triangles(ctx, 0, LRS_R, 1, F.triangleMinViol, nullptr, nullptr, nullptr, &nviol, &maxv) ||
        !record(t0, 0, 0, nviol, maxv)) {
        fprintf(stderr, "[lrsdp] cut rounds skipped: %s\n", lrs_last_error());
        rounds.clear();
        return;
    }
    std::vector<int> have, cand;
    std::vector<double> slack, lam;
    for (int rnd = 0; rnd < F.cutRounds; ++rnd) {
        t0 = now();
        lrs_cuts_get(ctx, nullptr, 0, &ncut);
        have.assign(4 * (size_t)(ncut > 0 ? ncut : 1), 0);
        slack.assign(ncut > 0 ? ncut : 1, 0.0);
        lam.assign(ncut > 0 ? ncut : 1, 0.0);
        lrs_cuts_get(ctx, have.data(), ncut, nullptr);
        if (lrs_cuts_state(ctx, LRS_R, slack.data(), lam.data())) break;
        int extra = 0;
        for (int t = 0; t < ncut; ++t) extra += slack[t] < -F.triangleMinViol ? 1 : 0;
        const int want = K + extra < LRS_TRI_MAX_K ? K + extra : LRS_TRI_MAX_K;
        cand.assign(4 * (size_t)want, 0);
        int got = 0;
        if (lrs_separate_triangles(ctx, 0, LRS_R, want, F.triangleMinViol, cand.data(), nullptr, &got, &nviol, &maxv)) break;
        std::vector<std::vector<int>> known;
        for (int t = 0; t < ncut; ++t) known.push_back({have[4 * t], have[4 * t + 1], have[4 * t + 2], have[4 * t + 3]});
        std::sort(known.begin(), known.end());
        std::vector<int> fresh;
        for (int t = 0; t < got && (int)fresh.size() < 4 * K; ++t) {
            const std::vector<int> q(cand.begin() + 4 * t, cand.begin() + 4 * t + 4);
            if (!std::binary_search(known.begin(), known.end(), q)) fresh.insert(fresh.end(), q.begin(), q.end());
        }
        if (fresh.empty()) break;
        int dropped = 0, added = 0;
        if (F.cutDrop && ncut > 0) {
            std::vector<unsigned char> mark(ncut, 0);
            for (int t = 0; t < ncut; ++t) mark[t] = slack[t] > F.cutDropSlack && lam[t] >= 0.0;
            if (lrs_cuts_drop(ctx, mark.data(), 1, &dropped)) break;
        }
        lrs_result rr;
        if (lrs_cuts_append(ctx, fresh.data(), (int)(fresh.size() / 4), 1, &added) ||
            (F.compressTol >= 0 && lrs_factor_compress(ctx, LRS_R, nullptr, F.compressTol, F.compressSlack, nullptr, nullptr,
                                                       nullptr, nullptr)) ||
            lrs_solve_warm(ctx, &F.p, &rr)) {
            fprintf(stderr, "[lrsdp] cut round %d failed: %s\n", rnd + 1, lrs_last_error());
            break;
        }
        rr.read_time = r.read_time;
        r = rr;
        if (!record(t0, added, dropped, nviol, maxv)) break;
    }
    if (!F.triangleFile.empty()) {
        lrs_cuts_get(ctx, nullptr, 0, &ncut);
        have.assign(4 * (size_t)(ncut > 0 ? ncut : 1), 0);
        slack.assign(ncut > 0 ? ncut : 1, 0.0);
        lrs_cuts_get(ctx, have.data(), ncut, nullptr);
        lrs_cuts_state(ctx, LRS_R, slack.data(), nullptr);
        FILE *f = fopen(F.triangleFile.c_str(), "w");
        if (!f) fprintf(stderr, "[lrsdp] cannot open %s\n", F.triangleFile.c_str());
        else {
            for (int t = 0; t < ncut; ++t)
                fprintf(f, "%d %d %d %d %.17g\n", have[4 * t] + 1, have[4 * t + 1] + 1, have[4 * t + 2] + 1, have[4 * t + 3],
                        -slack[t]);
            fclose(f);
        }
    }
}

// --batch FILE: load every line's instance, one lrs_solve_batch, one JSON each
// --compressTol t after the last solve: the final point compressed in the context, and the JSON at
// jsonFile (if any) gains "compressed" before its closing brace
static void compress_and_report(lrs_ctx *ctx, const Flags &F, const lrs_result &r, const char *jsonFile) {
    if (F.compressTol < 0) return;
    int m = 0, K = 0;
    lrs_problem_info(ctx, &m, &K, nullptr, nullptr, nullptr);
    std::vector<int> old(K > 0 ? K : 1, 0), nr(old);
    lrs_get_rank(ctx, old.data());
    size_t tot = 0;
    for (int k = 0; k < K; ++k) tot += (size_t)old[k];
    std::vector<double> eigs(tot ? tot : 1, 0.0), lost(old.size(), 0.0);
    const int which = (r.admm_iter > 0 || r.traj2_len > 0) ? LRS_U : LRS_R;
    if (lrs_factor_compress(ctx, which, nullptr, F.compressTol, F.compressSlack, nr.data(), eigs.data(), lost.data(),
                            nullptr)) {
        fprintf(stderr, "[lrsdp] compression skipped: %s\n", lrs_last_error());
        return;
    }
    auto num = [](double v) {
        char b[40];
        snprintf(b, sizeof(b), "%.16e", v);
        return std::string(b);
    };
    std::string ranks, lt, sp;
    size_t off = 0;
    int before = 0, after = 0;
    for (int k = 0; k < K; ++k) {
        ranks += (k ? ", " : "") + std::to_string(nr[k]);
        lt += (k ? ", " : "") + num(lost[k]);
        sp += k ? ", [" : "[";
        for (int j = 0; j < old[k]; ++j) sp += (j ? ", " : "") + num(eigs[off + j]);
        sp += "]";
        off += (size_t)old[k];
        before += old[k];
        after += nr[k];
    }
    printf("Compression (%s, tol %g, slack %d): rank %d -> %d\n", which == LRS_U ? "(U+V)/2" : "R", F.compressTol,
           F.compressSlack, before, after);
    if (jsonFile)
        json_append(jsonFile, ",\n  \"compressed\": {\"ranks\": [" + ranks + "], \"lost_trace\": [" + lt +
                                  "], \"spectrum\": [" + sp + "]}\n}\n");
}

static int run_batch(const Flags &base, const char *prog) {
    FILE *f = fopen(base.batchFile.c_str(), "r");
    if (!f) {
        fprintf(stderr, "[lrsdp] cannot open batch file %s\n", base.batchFile.c_str());
        return 1;
    }
    struct Job {
        Flags F;
        std::string inst;
        std::vector<int> sched;
        lrs_ctx *ctx = nullptr;
        bool ok = false;
    };
    std::vector<Job *> jobs;
    bool cut_flag = base.cutRounds > 0;
    std::string text;
    char buf[4096];
    size_t nr;
    while ((nr = fread(buf, 1, sizeof(buf), f)) > 0) text.append(buf, nr);
    fclose(f);
    int failed = 0;
    for (size_t pos = 0; pos < text.size();) {
        size_t e = text.find('\n', pos);
        if (e == std::string::npos) e = text.size();
        std::string line = text.substr(pos, e - pos);
        pos = e + 1;
        std::vector<std::string> tok;
        for (size_t i = 0; i < line.size();) {
            while (i < line.size() && isspace((unsigned char)line[i])) i++;
            size_t j = i;
            while (j < line.size() && !isspace((unsigned char)line[j])) j++;
            if (j > i) tok.push_back(line.substr(i, j - i));
            i = j;
        }
        if (tok.empty()) continue;
        if (tok.size() < 2) {
            fprintf(stderr, "[lrsdp] batch line `%s`: expected <instance.dat-s> <jsonfile> [flags...]\n", line.c_str());
            failed++;
            continue;
        }
        Job *j = new Job();
        j->F = base;
        j->F.batchFile.clear();
        j->inst = tok[0];
        std::vector<char *> av;
        av.push_back(const_cast<char *>(prog));
        for (size_t q = 2; q < tok.size(); ++q) av.push_back(const_cast<char *>(tok[q].c_str()));
        av.push_back(nullptr);
        parse_flags((int)av.size() - 1, av.data(), j->F);
        j->F.jsonFile = tok[1];
        finish_flags(j->F, j->sched);
        cut_flag = cut_flag || j->F.cutRounds > 0;
        jobs.push_back(j);
    }
    if (cut_flag) fprintf(stderr, "[lrsdp] --cutRounds is ignored with --batch\n");
    if ((int)jobs.size() > LRS_BATCH_MAX) {
        fprintf(stderr, "[lrsdp] batch file %s: %zu instances (at most %d)\n", base.batchFile.c_str(), jobs.size(),
                LRS_BATCH_MAX);
        return 1;
    }
    std::vector<lrs_ctx *> ctxs;
    std::vector<lrs_params> prm;
    std::vector<Job *> live;
    for (Job *j : jobs) {
        if (lrs_ctx_create(base.device, &j->ctx) || lrs_load_sdpa(j->ctx, j->inst.c_str(), nullptr)) {
            fprintf(stderr, "[lrsdp] batch: %s failed: %s\n", j->inst.c_str(), lrs_last_error());
            failed++;
            continue;
        }
        if (!j->F.logFile.empty() && j->F.logFile != base.logFile) lrs_set_log_path(j->ctx, j->F.logFile.c_str());
        ctxs.push_back(j->ctx);
        prm.push_back(j->F.p);
        live.push_back(j);
    }
    if (!live.empty()) {
        lrs_batch *b = nullptr;
        std::vector<lrs_result> res(live.size());
        std::vector<int> rc(live.size(), 0);
        if (lrs_batch_create(&b)) {
            fprintf(stderr, "[lrsdp] %s\n", lrs_last_error());
            return 1;
        }
        const int ret = lrs_solve_batch(b, ctxs.data(), (int)live.size(), prm.data(), (int)live.size(), res.data(), rc.data());
        if (ret && lrs_last_error()[0] && !rc.empty()) {
            bool any = false;
            for (int v : rc) any = any || v != 0;
            if (!any) {   // the call itself was refused
                fprintf(stderr, "[lrsdp] batch: %s\n", lrs_last_error());
                failed += (int)live.size();
                live.clear();
            }
        }
        for (size_t q = 0; q < live.size(); ++q) {
            Job *j = live[q];
            if (rc[q]) {
                fprintf(stderr, "[lrsdp] batch: %s failed: %s\n", j->inst.c_str(), lrs_batch_error(b, (int)q));
                failed++;
                continue;
            }
            const std::string pid = problem_name(j->inst.c_str());
            if (lrs_write_json(j->ctx, j->F.jsonFile.c_str(), pid.c_str(), j->inst.c_str(), &res[q], &j->F.p)) {
                fprintf(stderr, "[lrsdp] batch: %s failed: %s\n", j->inst.c_str(), lrs_last_error());
                failed++;
                continue;
            }
            printf("%s: pObj %10.6e dObj %10.6e ALM inner %ld ADMM %ld all_time %f -> %s\n", pid.c_str(), res[q].pobj,
                   res[q].dobj, res[q].alm_inner, res[q].admm_iter, res[q].solve_time, j->F.jsonFile.c_str());
            round_and_report(j->ctx, j->F, j->F.jsonFile.c_str());   // each member on its own stream
            triangles_and_report(j->ctx, j->F, j->F.jsonFile.c_str());
        }
        long launches = 0, served = 0, alone = 0;
        int widest = 0;
        lrs_batch_stats(b, &launches, &widest, &served, &alone);
        printf("batch: %zu instances, %ld combined launches (widest round %d), %ld inner-loop calls served, %ld alone\n",
               live.size(), launches, widest, served, alone);
        lrs_batch_admm_stats(b, &launches, &widest, &served, &alone);
        printf("batch ADMM: %ld combined launches (widest round %d members), %ld iterations served, %ld alone\n",
               launches, widest, served, alone);
        lrs_batch_destroy(b);
    }
    for (Job *j : jobs) {
        if (j->ctx) lrs_ctx_destroy(j->ctx);
        delete j;
    }
    if (failed) fprintf(stderr, "[lrsdp] batch: %d instance(s) failed\n", failed);
    return failed ? 1 : 0;
}

int main(int argc, char **argv) {
    Flags F;
    lrs_params_default(&F.p);
    F.p.verbose = 1;
    if (argc < 2) {
        fprintf(stderr, "usage: %s <file.dat-s> [--flag value ...]\n       %s --batch FILE [--flag value ...]\n", argv[0],
                argv[0]);
        return 0;
    }
    const char *fname = argv[1];
    parse_flags(argc, argv, F);
    std::vector<int> sched;
    if (!F.batchFile.empty()) return run_batch(F, argv[0]);
    finish_flags(F, sched);
    lrs_params &p = F.p;
    const char *logFile = F.logFile.empty() ? nullptr : F.logFile.c_str();
    const char *jsonFile = F.jsonFile.empty() ? nullptr : F.jsonFile.c_str();
    const int device = F.device;
    printf("-----------------------------------------------------------\n");
    printf("  LoRADS-compatible low-rank SDP solver on MI355X (%s)\n", lrs_version());
    printf("-----------------------------------------------------------\n");
    lrs_ctx *ctx = nullptr;
    if (lrs_ctx_create(device, &ctx)) {
        fprintf(stderr, "[lrsdp] %s\n", lrs_last_error());
        return 0;
    }
    if (logFile) lrs_set_log_path(ctx, logFile);
    double tread = 0;
    if (lrs_load_sdpa(ctx, fname, &tread)) {
        fprintf(stderr, "[lrsdp] %s\n", lrs_last_error());
        lrs_ctx_destroy(ctx);
        return 0;   // main.c:383-385 exits 0 on read failure too
    }
    int m = 0, K = 0;
    lrs_problem_info(ctx, &m, &K, nullptr, nullptr, nullptr);
    printf("Reading SDPA file in %f seconds \n", tread);
    printf("nConstrs = %d, sdp nBlks = %d, lp Cols = %d\n", m, K, 0);
    if (F.rankShrink > 0 && lrs_set_rank_shrink(ctx, F.rankShrink, F.compressSlack))
        fprintf(stderr, "[lrsdp] --rankShrink ignored: %s\n", lrs_last_error());
    lrs_result r;
    if (lrs_solve(ctx, &p, &r)) {
        fprintf(stderr, "[lrsdp] solve failed: %s\n", lrs_last_error());
        lrs_ctx_destroy(ctx);
        return 0;
    }
    std::string rounds;
    const bool cut_mode = F.cutRounds > 0;
    if (cut_mode && F.triangleCuts <= 0) fprintf(stderr, "[lrsdp] --cutRounds needs --triangleCuts K; ignored\n");
    else if (cut_mode) cut_rounds(ctx, F, r, rounds);
    printf("-----------------------------------------------------------------------\n");
    // LORADSEndProgram, data/lorads_solver.c:1307-1333
    if (r.status == 3) printf("End Program due to reaching `the maximum number of iterations`:\n");
    else if (r.status == 1) printf("End Program due to reaching `Official terminate criteria`:\n");
    else if (r.status == 2) printf("End Program due to reaching `final terminate criteria`:\n");
    else if (r.status == 4) printf("End Program since time limit.\n");
    else printf("End Program but the status is unknown, please notify the authors\n");
    const double dinf = r.dinf < 0 ? 0.0 : r.dinf, dinf_inf = r.dinf_inf < 0 ? 0.0 : r.dinf_inf;
    printf("Objective function Value are:\n");
    printf("\t 1.Primal Objective:            : %10.6e\n", r.pobj);
    printf("\t 2.Dual Objective:              : %10.6e\n", r.dobj);
    printf("Dimacs Error are:\n");
    printf("\t 1.Constraint Violation(1)      : %10.6e\n", r.pinf);
    printf("\t 2.Dual Infeasibility(1)        : %10.6e\n", dinf);
    printf("\t 3.Primal Dual Gap              : %10.6e\n", r.gap);
    printf("\t 4.Primal Variable Semidefinite : %10.6e\n", 0.0);
    printf("\t 5.Constraint Violation(Inf)    : %10.6e\n", r.pinf_inf);
    printf("\t 6.Dual Infeasibility(Inf)      : %10.6e\n", dinf_inf);
    printf("-----------------------------------------------------------------------\n");
    printf("ALM inner iterations: %ld, ALM time: %f s, ADMM iterations: %ld\n", r.alm_inner, r.alm_time, r.admm_iter);
    printf("all_time: %f\n", r.solve_time);
    if (jsonFile) {
        std::string pid = problem_name(fname);
        if (lrs_write_json(ctx, jsonFile, pid.c_str(), fname, &r, &p))
            fprintf(stderr, "[lrsdp] %s\n", lrs_last_error());
        else
            printf("JSON output written to: %s\n", jsonFile);
    }
    round_and_report(ctx, F, jsonFile, !rounds.empty());
    // after cut rounds the triangles' report is the rounds' (the file holds the final cut list)
    if (rounds.empty()) triangles_and_report(ctx, F, jsonFile);
    else if (jsonFile) json_append(jsonFile, ",\n  \"cut_rounds\": [" + rounds + "\n  ]\n}\n");
    compress_and_report(ctx, F, r, jsonFile);
    lrs_ctx_destroy(ctx);
    return 0;
}
