// Stand-alone test of a batched solve's two meetings (ltr-lowrank-sdp_amd/csrc/lrs_batch_rdv.h):
// one BatchRendezvous for the ALM phase and a second, independent one for the ADMM phase, with
// stubs in place of the combined launches: no GPU, no library.  One host thread a member, as
// lrs_solve_batch runs them: every member starts in the first quorum, leaves it after its ALM
// calls and then, if its ADMM iteration qualifies, joins the second quorum for its ADMM calls
// (a scope guard, as admm_optimize); a member that does not qualify makes those calls alone.
// Members move at different times.  Checked: every call is served exactly once by a round of
// its own meeting; a round's members are exactly the members parked in that meeting at that
// moment; one round at a time per meeting; the first meeting's widths are what the lengths
// imply; a member in one phase never waits for a member in the other (two scenarios that could
// not end otherwise); the counters of each meeting count its own rounds only; the program ends
// (the pytest wrapper gives it a time limit).  Exit code 0 and "ok" on success.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../../ltr-lowrank-sdp_amd/csrc/lrs_batch_rdv.h"

#define CHECK(x)                                                              \
    do {                                                                      \
        if (!(x)) {                                                           \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #x); \
            exit(1);                                                          \
        }                                                                     \
    } while (0)

// where a member is: outside both quorums, or in meeting q (0 ALM, 1 ADMM) idle / parked
enum State { OUT = 0, IN0 = 1, PARKED0 = 2, IN1 = 3, PARKED1 = 4 };

struct Member {
    int alm = 0;               // calls to the first meeting
    int admm = 0;              // ADMM iterations
    bool joins = true;         // false: its ADMM iterations run alone, never in the second quorum
    int fail_admm_after = -1;  // >= 0: an error return out of the ADMM phase after that many calls
    // >= 0: waits (outside any submit) for that member to have finished, before leaving the first
    // quorum (hold_alm) or, inside the second quorum, before its first ADMM call (hold_admm)
    int hold_alm_for = -1, hold_admm_for = -1;
};

struct Scenario {
    std::vector<Member> mem;
    int admm_stub_fails_at = -1;   // >= 0: the second meeting's stub fails in that round
};

struct Outcome {
    std::vector<int> w0, w1;   // the widths of the two meetings' rounds, in order
    int overlap = 0;           // rounds of the second meeting that began while one of the first ran
};

static Outcome run(const Scenario &sc) {
    const int n = (int)sc.mem.size();
    lrs::BatchRendezvous rdv[2];
    std::vector<std::atomic<int>> state(n), done(n);
    std::vector<std::atomic<long>> served0(n), served1(n), alone(n);
    std::vector<long> sub0(n, 0), sub1(n, 0), got_err(n, 0);
    for (int i = 0; i < n; ++i) { state[i] = OUT; done[i] = 0; served0[i] = 0; served1[i] = 0; alone[i] = 0; }
    Outcome out;
    std::atomic<int> in_round[2];
    in_round[0] = 0; in_round[1] = 0;
    for (int q = 0; q < 2; ++q)
        rdv[q].reset(n, [&, q](const std::vector<int> &m) -> int {
            CHECK(in_round[q].fetch_add(1) == 0);   // one round at a time in a meeting
            if (q == 1 && in_round[0].load() > 0) out.overlap++;
            CHECK(!m.empty());
            const int parked_state = q ? PARKED1 : PARKED0;
            // the round's members are exactly the members parked in THIS meeting; members of the
            // other meeting, parked or not, are none of its business
            int parked = 0;
            for (int i = 0; i < n; ++i) parked += state[i] == parked_state;
            for (size_t k = 0; k < m.size(); ++k) {
                CHECK(m[k] >= 0 && m[k] < n && state[m[k]] == parked_state);
                if (k) CHECK(m[k] > m[k - 1]);
                (q ? served1 : served0)[m[k]]++;
            }
            // (the first quorum only shrinks, so its count is exact; a member may join the second
            // quorum and reach its first call while a round of it runs: that one waits its turn)
            if (q == 0) CHECK(parked == (int)m.size());
            else CHECK(parked >= (int)m.size());
            std::vector<int> &w = q ? out.w1 : out.w0;
            const int r = (int)w.size();
            w.push_back((int)m.size());
            std::this_thread::yield();
            CHECK(in_round[q].fetch_sub(1) == 1);
            return (q == 1 && r == sc.admm_stub_fails_at) ? -9 : 0;
        });
    // as lrs_solve_batch: everyone counts towards the first quorum, nobody towards the second
    for (int i = 0; i < n; ++i) {
        rdv[0].enter(i);
        state[i] = IN0;
    }
    auto wait_for = [&](int j) {
        while (!done[j].load()) std::this_thread::yield();
    };
    std::vector<std::thread> th;
    for (int i = 0; i < n; ++i)
        th.emplace_back([&, i] {
            const Member &me = sc.mem[i];
            {
                lrs::BatchRendezvous::Scope scope(&rdv[0], i, true);   // idempotent: already entered
                for (int r = 0; r < me.alm; ++r) {
                    state[i] = PARKED0;
                    sub0[i]++;
                    CHECK(rdv[0].submit(i) == 0);
                    state[i] = IN0;
                    CHECK(served0[i] == r + 1);
                }
                if (me.hold_alm_for >= 0) wait_for(me.hold_alm_for);
                state[i] = OUT;
            }
            CHECK(!rdv[0].in_quorum(i) && !rdv[1].in_quorum(i));
            if (!me.joins) {
                for (int r = 0; r < me.admm; ++r) alone[i]++;
            } else {
                // admm_optimize: in the second quorum from its entry to every exit
                lrs::BatchRendezvous::Scope scope(&rdv[1], i, true);
                state[i] = IN1;
                if (me.hold_admm_for >= 0) wait_for(me.hold_admm_for);
                for (int r = 0; r < me.admm; ++r) {
                    if (r == me.fail_admm_after) break;   // an error return: the guard leaves
                    state[i] = PARKED1;
                    sub1[i]++;
                    const int rc = rdv[1].submit(i);
                    state[i] = IN1;
                    CHECK(served1[i] == r + 1);
                    if (rc) { CHECK(rc == -9); got_err[i]++; break; }
                }
                state[i] = OUT;
            }
            CHECK(!rdv[1].in_quorum(i));
            rdv[0].leave(i);   // as the member's thread does after its solve
            rdv[1].leave(i);
            done[i] = 1;
        });
    for (auto &t : th) t.join();
    long s0 = 0, s1 = 0, t0 = 0, t1 = 0;
    for (int i = 0; i < n; ++i) {
        CHECK(served0[i] == sub0[i] && served1[i] == sub1[i]);
        CHECK(sc.mem[i].joins || (served1[i] == 0 && alone[i] == sc.mem[i].admm));
        s0 += sub0[i];
        s1 += sub1[i];
    }
    int wd0 = 0, wd1 = 0;
    for (int w : out.w0) { t0 += w; wd0 = std::max(wd0, w); }
    for (int w : out.w1) { t1 += w; wd1 = std::max(wd1, w); }
    CHECK(t0 == s0 && t1 == s1);
    // each meeting's counters count its own rounds only
    for (int q = 0; q < 2; ++q) {
        long rounds = 0, srv = 0;
        int wd = 0;
        rdv[q].stats(&rounds, &wd, &srv);
        CHECK(rounds == (long)(q ? out.w1 : out.w0).size() && wd == (q ? wd1 : wd0) && srv == (q ? s1 : s0));
        const std::vector<long> h = rdv[q].width_histogram();
        long hs = 0;
        for (size_t w = 0; w < h.size(); ++w) hs += (long)w * h[w];
        CHECK(hs == (q ? s1 : s0));
    }
    if (sc.admm_stub_fails_at >= 0 && (int)out.w1.size() > sc.admm_stub_fails_at) {
        long errs = 0;
        for (int i = 0; i < n; ++i) errs += got_err[i];
        CHECK(errs == out.w1[sc.admm_stub_fails_at]);   // every member of the failed round got its code
    }
    return out;
}

// the first meeting: round k runs every member that makes more than k ALM calls
static std::vector<int> expected_alm(const Scenario &sc) {
    std::vector<int> w;
    for (int k = 0;; ++k) {
        int c = 0;
        for (const Member &m : sc.mem) c += m.alm > k;
        if (!c) break;
        w.push_back(c);
    }
    return w;
}

int main() {
    // members that move from the first quorum to the second at different times, three of them
    // never joining the second: the first meeting's widths are fixed by the lengths; the second
    // meeting's depend on who has arrived, but every call is served once and the program ends
    {
        Scenario sc;
        for (int i = 0; i < 13; ++i) {
            Member m;
            m.alm = 1 + (i * 5) % 7;
            m.admm = 3 + (i * 3) % 9;
            m.joins = i % 4 != 3;
            sc.mem.push_back(m);
        }
        int overlaps = 0;
        for (int rep = 0; rep < 200; ++rep) {
            const Outcome o = run(sc);
            CHECK(o.w0 == expected_alm(sc));
            for (int w : o.w1) CHECK(w >= 1 && w <= 10);   // 10 of the 13 ever join
            overlaps += o.overlap;
        }
        (void)overlaps;   // rounds of the two meetings may run at the same time; nothing requires it
    }
    // equal ALM lengths: everyone reaches the second quorum after the same round
    {
        Scenario sc;
        for (int i = 0; i < 6; ++i) {
            Member m;
            m.alm = 3;
            m.admm = 10;
            sc.mem.push_back(m);
        }
        for (int rep = 0; rep < 50; ++rep) {
            const Outcome o = run(sc);
            CHECK(o.w0 == expected_alm(sc));
            long tot = 0;
            for (int w : o.w1) tot += w;
            CHECK(tot == 60);
        }
    }
    // a member in ADMM never waits for a member in ALM: member 1 stays in the first quorum (idle,
    // not parked) until member 0 has finished its whole ADMM phase, then runs its own
    {
        Scenario sc;
        Member a, b;
        a.alm = 1; a.admm = 5;
        b.alm = 1; b.admm = 5; b.hold_alm_for = 0;
        sc.mem = {a, b};
        for (int rep = 0; rep < 50; ++rep) {
            const Outcome o = run(sc);
            CHECK(o.w0 == std::vector<int>({2}));
            CHECK(o.w1 == std::vector<int>(10, 1));
        }
    }
    // a member in ALM never waits for a member in ADMM: member 0 sits in the second quorum (idle,
    // not parked) until member 1 has finished, whose ALM rounds run meanwhile, one member wide;
    // member 1's ADMM rounds then wait for nobody either way: member 0 is idle in that quorum
    // only until member 1 is done, so member 1 does not join it (its iterations run alone)
    {
        Scenario sc;
        Member a, b;
        a.alm = 1; a.admm = 4; a.hold_admm_for = 1;
        b.alm = 6; b.admm = 3; b.joins = false;
        sc.mem = {a, b};
        for (int rep = 0; rep < 50; ++rep) {
            const Outcome o = run(sc);
            CHECK(o.w0 == std::vector<int>({2, 1, 1, 1, 1, 1}));
            CHECK(o.w1 == std::vector<int>(4, 1));
        }
    }
    // an error return out of the ADMM phase between rounds (the guard leaves the quorum), and a
    // member with no ADMM iteration at all: nobody is left waiting
    {
        Scenario sc;
        Member a, b, c, d;
        a.alm = 2; a.admm = 8;
        b.alm = 2; b.admm = 8; b.fail_admm_after = 3;
        c.alm = 2; c.admm = 0;
        d.alm = 4; d.admm = 6; d.joins = false;
        sc.mem = {a, b, c, d};
        for (int rep = 0; rep < 200; ++rep) {
            const Outcome o = run(sc);
            CHECK(o.w0 == expected_alm(sc));
            long tot = 0;
            for (int w : o.w1) tot += w;
            CHECK(tot == 8 + 3);
        }
    }
    // a failing ADMM round: its members all get the code and leave; the first meeting's rounds
    // of the members still in ALM are untouched
    {
        Scenario sc;
        for (int i = 0; i < 5; ++i) {
            Member m;
            m.alm = 2;
            m.admm = 4 + i;
            sc.mem.push_back(m);
        }
        Member late;
        late.alm = 9; late.admm = 2; late.hold_alm_for = 0;
        sc.mem.push_back(late);
        sc.admm_stub_fails_at = 0;
        for (int rep = 0; rep < 50; ++rep) {
            const Outcome o = run(sc);
            CHECK(o.w0 == expected_alm(sc));
            CHECK(!o.w1.empty());
        }
    }
    printf("ok\n");
    return 0;
}
