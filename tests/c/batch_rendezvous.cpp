// Stand-alone test of the batched solve's rendezvous (ltr-lowrank-sdp_amd/csrc/lrs_batch_rdv.h)
// with a stub in place of the combined launch: no GPU, no library.  One host thread a member,
// as lrs_solve_batch runs them.  Checked: every submitted call is served exactly once, a
// round's members are exactly the quorum at that moment (all of them parked), the widths of
// the rounds are what the members' lengths imply, and the program ends (the pytest wrapper
// gives it a time limit).  Exit code 0 and "ok" on success; the first failed check aborts.
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

enum State { OUT = 0, IN = 1, PARKED = 2, RUNNING = 3 };

struct Member {
    int rounds = 0;            // inner-loop calls it submits when nothing stops it
    bool never = false;        // takes another inner loop: leaves the quorum before any call
    bool fail_first = false;   // fails before its first submit
    int fail_after = -1;       // >= 0: fails after that many served calls
};

struct Scenario {
    std::vector<Member> mem;
    int stub_fails_at = -1;    // >= 0: the stub returns an error in that round
};

// Runs the scenario once; returns the widths of its rounds in order.
static std::vector<int> run(const Scenario &sc) {
    const int n = (int)sc.mem.size();
    lrs::BatchRendezvous rdv;
    std::vector<std::atomic<int>> state(n);
    std::vector<std::atomic<long>> served(n), alone(n);
    std::vector<long> submitted(n, 0), got_err(n, 0);
    for (int i = 0; i < n; ++i) { state[i] = OUT; served[i] = 0; alone[i] = 0; }
    std::vector<int> widths;
    std::atomic<int> in_round{0};
    rdv.reset(n, [&](const std::vector<int> &m) -> int {
        CHECK(in_round.fetch_add(1) == 0);   // one round at a time
        CHECK(!m.empty());
        // the round's members are exactly the parked ones, and nobody who was in the quorum
        // before this round is still running (IN is a member that has only just joined or is
        // about to take its first decision: it may enter while a round runs)
        int parked = 0, running = 0;
        for (int i = 0; i < n; ++i) {
            parked += state[i] == PARKED;
            running += state[i] == RUNNING;
        }
        for (size_t q = 0; q < m.size(); ++q) {
            CHECK(m[q] >= 0 && m[q] < n && state[m[q]] == PARKED);
            if (q) CHECK(m[q] > m[q - 1]);
            served[m[q]]++;
        }
        CHECK(parked == (int)m.size());
        CHECK(running == 0);
        const int r = (int)widths.size();
        widths.push_back((int)m.size());
        std::this_thread::yield();
        CHECK(in_round.fetch_sub(1) == 1);
        return r == sc.stub_fails_at ? -7 : 0;
    });
    // as lrs_solve_batch: everyone counts until its solve decides otherwise
    bool any_first = false;
    for (int i = 0; i < n; ++i) {
        rdv.enter(i);
        state[i] = IN;
        any_first = any_first || (!sc.mem[i].never && !sc.mem[i].fail_first && sc.mem[i].rounds > 0);
    }
    std::vector<std::thread> th;
    for (int i = 0; i < n; ++i)
        th.emplace_back([&, i] {
            const Member &me = sc.mem[i];
            if (me.fail_first) { state[i] = OUT; rdv.leave(i); return; }
            if (me.never) {
                state[i] = OUT;
                rdv.leave(i);
                for (int r = 0; r < me.rounds; ++r) alone[i]++;
                return;
            }
            {
                lrs::BatchRendezvous::Scope scope(&rdv, i, true);   // idempotent: already entered
                for (int r = 0; r < me.rounds; ++r) {
                    if (r == me.fail_after) break;
                    state[i] = PARKED;
                    submitted[i]++;
                    const int rc = rdv.submit(i);
                    state[i] = RUNNING;
                    CHECK(served[i] == r + 1);   // served exactly once per call, before submit returns
                    if (rc) { CHECK(rc == -7); got_err[i]++; break; }
                }
                state[i] = OUT;
            }
            CHECK(!rdv.in_quorum(i));
        });
    for (auto &t : th) t.join();
    long tot = 0, sub = 0;
    for (int i = 0; i < n; ++i) {
        CHECK(served[i] == submitted[i]);
        CHECK(!sc.mem[i].never || (served[i] == 0 && alone[i] == sc.mem[i].rounds));
        CHECK(!sc.mem[i].fail_first || served[i] == 0);
        sub += submitted[i];
    }
    int widest = 0;
    for (int w : widths) { tot += w; widest = std::max(widest, w); }
    CHECK(tot == sub);
    long rounds = 0, srv = 0;
    int wd = 0;
    rdv.stats(&rounds, &wd, &srv);
    CHECK(rounds == (long)widths.size() && wd == widest && srv == sub);
    const std::vector<long> h = rdv.width_histogram();
    long hs = 0;
    for (size_t w = 0; w < h.size(); ++w) hs += (long)w * h[w];
    CHECK(hs == sub);
    if (sc.stub_fails_at >= 0 && (int)widths.size() > sc.stub_fails_at) {
        long errs = 0;
        for (int i = 0; i < n; ++i) errs += got_err[i];
        CHECK(errs == widths[sc.stub_fails_at]);   // every member of the failed round got its code
    }
    return widths;
}

// round k runs every member that submits more than k calls
static std::vector<int> expected(const Scenario &sc) {
    std::vector<int> w;
    for (int k = 0;; ++k) {
        int c = 0;
        for (const Member &m : sc.mem) {
            if (m.never || m.fail_first) continue;
            const int len = m.fail_after >= 0 ? std::min(m.rounds, m.fail_after) : m.rounds;
            c += len > k;
        }
        if (!c) break;
        w.push_back(c);
    }
    return w;
}

int main() {
    // 1, 2 and 17 members of equal length: every round has them all
    for (int n : {1, 2, 17}) {
        Scenario sc;
        sc.mem.assign(n, Member{20});
        for (int rep = 0; rep < 20; ++rep) {
            const std::vector<int> w = run(sc);
            CHECK(w.size() == 20);
            for (int x : w) CHECK(x == n);
        }
    }
    // members leaving after different numbers of rounds
    {
        Scenario sc;
        for (int i = 0; i < 17; ++i) sc.mem.push_back(Member{1 + (i * 7) % 11});
        for (int rep = 0; rep < 200; ++rep) CHECK(run(sc) == expected(sc));
    }
    // a member that fails before its first submit, one that fails between rounds, one that is
    // never in the quorum (it makes its calls alone), three ordinary ones
    {
        Scenario sc;
        Member a{4}, b{4}, c{6};
        a.fail_first = true;
        b.fail_after = 2;
        c.never = true;
        sc.mem = {a, b, c, Member{4}, Member{4}, Member{5}};
        const std::vector<int> want = {4, 4, 3, 3, 1};
        CHECK(expected(sc) == want);
        for (int rep = 0; rep < 200; ++rep) CHECK(run(sc) == want);
    }
    // nobody ever submits: the call ends all the same
    {
        Scenario sc;
        Member a{3}, c{2};
        a.fail_first = true;
        c.never = true;
        sc.mem = {a, c, a};
        for (int rep = 0; rep < 20; ++rep) CHECK(run(sc).empty());
    }
    // a round that fails: its members all get the code and leave; nobody is left waiting
    {
        Scenario sc;
        for (int i = 0; i < 5; ++i) sc.mem.push_back(Member{3 + i});
        sc.stub_fails_at = 1;
        for (int rep = 0; rep < 50; ++rep) {
            const std::vector<int> w = run(sc);
            CHECK(w.size() == 2 && w[0] == 5 && w[1] == 5);
        }
    }
    printf("ok\n");
    return 0;
}
