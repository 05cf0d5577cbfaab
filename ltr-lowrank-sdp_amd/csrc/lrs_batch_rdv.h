// lrs_batch_rdv.h -- the rendezvous of a batched solve (lrs_solve_batch).
// Host-only: no device call in here; the round (the combined launches and the wait for
// them) is a callback, so tests/c/batch_rendezvous.cpp drives the class without a GPU.
//
// Every member of a batch runs its own solve on a host thread of its own.  The members
// currently inside the ALM phase on the single-workgroup inner loop form the quorum
// (enter / leave; Scope is the guard).  A quorum member's inner-loop call does not launch:
// it submits and parks.  When every quorum member is parked one of them runs the round over
// all parked members and wakes them.  A departure re-evaluates "everyone parked", so nobody
// waits on a member that is gone.  The only waits: a member reaching enter / leave / submit,
// and whatever the callback itself waits for (the batch streams).
#ifndef LRS_BATCH_RDV_H
#define LRS_BATCH_RDV_H
#include <algorithm>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <vector>

namespace lrs {

class BatchRendezvous {
public:
    // the round over the parked members (ascending member indices): returns 0, or non-zero
    // when the round failed -- every member of that round then gets that code from submit()
    using RoundFn = std::function<int(const std::vector<int> &)>;

    void reset(int n, RoundFn fn) {
        std::lock_guard<std::mutex> lk(mu_);
        n_ = n;
        fn_ = std::move(fn);
        in_.assign(n, 0); parked_.assign(n, 0); served_.assign(n, 0); rc_.assign(n, 0);
        nquorum_ = nparked_ = 0;
        running_ = false;
        rounds_ = served_total_ = 0;
        widest_ = 0;
        hist_.assign(n + 1, 0);
    }
    // member i joins the quorum (idempotent)
    void enter(int i) {
        std::lock_guard<std::mutex> lk(mu_);
        if (!in_[i]) { in_[i] = 1; nquorum_++; }
    }
    // member i leaves the quorum (idempotent; never called while i is parked: a parked member
    // is inside submit()).  The rest may now all be parked: wake them, one takes the round.
    void leave(int i) {
        std::lock_guard<std::mutex> lk(mu_);
        if (!in_[i]) return;
        in_[i] = 0;
        nquorum_--;
        if (nparked_ > 0 && nparked_ == nquorum_) cv_.notify_all();
    }
    bool in_quorum(int i) {
        std::lock_guard<std::mutex> lk(mu_);
        return in_[i] != 0;
    }
    // member i (in the quorum) parks until a round has served it; returns that round's code
    int submit(int i) {
        std::unique_lock<std::mutex> lk(mu_);
        parked_[i] = 1;
        served_[i] = 0;
        nparked_++;
        while (!served_[i]) {
            if (!running_ && nparked_ == nquorum_) {
                running_ = true;
                std::vector<int> mem;
                for (int q = 0; q < n_; ++q)
                    if (parked_[q]) mem.push_back(q);
                lk.unlock();
                const int rc = fn_(mem);
                lk.lock();
                for (int q : mem) { parked_[q] = 0; served_[q] = 1; rc_[q] = rc; }
                nparked_ -= (int)mem.size();
                rounds_++;
                served_total_ += (long)mem.size();
                widest_ = std::max(widest_, (int)mem.size());
                hist_[mem.size()]++;
                running_ = false;
                cv_.notify_all();
            } else {
                cv_.wait(lk);
            }
        }
        return rc_[i];
    }
    // counters since reset(): rounds, the widest one, calls served; rounds by width
    void stats(long *rounds, int *widest, long *served) {
        std::lock_guard<std::mutex> lk(mu_);
        if (rounds) *rounds = rounds_;
        if (widest) *widest = widest_;
        if (served) *served = served_total_;
    }
    std::vector<long> width_histogram() {
        std::lock_guard<std::mutex> lk(mu_);
        return hist_;
    }

    // leaves the quorum on every exit from the scope that entered it
    struct Scope {
        BatchRendezvous *r;
        int i;
        Scope(BatchRendezvous *r_, int i_, bool join) : r(join ? r_ : nullptr), i(i_) { if (r) r->enter(i); }
        ~Scope() { if (r) r->leave(i); }
        Scope(const Scope &) = delete;
        Scope &operator=(const Scope &) = delete;
    };

private:
    std::mutex mu_;
    std::condition_variable cv_;
    RoundFn fn_;
    int n_ = 0, nquorum_ = 0, nparked_ = 0, widest_ = 0;
    bool running_ = false;
    long rounds_ = 0, served_total_ = 0;
    std::vector<char> in_, parked_, served_;
    std::vector<int> rc_;
    std::vector<long> hist_;
};

}  // namespace lrs
#endif
