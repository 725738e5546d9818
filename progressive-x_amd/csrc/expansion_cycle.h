// expansion_cycle.h — which moves of pgx_expansion's cycles are run, enqueued, skipped, restored or run again, and when a call need
// not run at all.  The level above move_route.h, and like it without HIP: libpgx.so (expansion.hip) and the CPU tests
// (tests/emu/mf_emu.cpp, tests/test_expansion_cycle.py, tests/emu/expansion_cycle_driver.cpp) compile the same code.  Everything that
// touches the device is behind the backend of run_expansion.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace pgx {

// A move is a deterministic function of (labelling, alpha): one that relabelled nothing and has seen no label change since would
// relabel nothing again and is skipped (typically the tail of the verifying cycle).  `version` counts the moves that relabelled
// something; noop_at[alpha] is the version at which alpha's last move relabelled nothing (-1: it relabelled, or never ran).
struct SkipRule {
    int64_t version = 0;
    std::vector<int64_t> noop_at;
    explicit SkipRule(int L) : noop_at((size_t)(L > 0 ? L : 1), -1) {}
    bool noop_now(int alpha) const { return noop_at[(size_t)alpha] == version; }
    void record(int alpha, int64_t changed)
    {
        if (changed > 0) { ++version; noop_at[(size_t)alpha] = -1; }
        else noop_at[(size_t)alpha] = version;
    }
    // For a move enqueued behind others of a batch opened at version0 (their outcome is not known yet): the device skips it if exactly
    // this many moves of the batch before it relabelled something; -1: it always runs.
    int skip_rel(int alpha, int64_t version0) const
    {
        return noop_at[(size_t)alpha] >= version0 ? (int)(noop_at[(size_t)alpha] - version0) : -1;
    }
};

// What an expansion was computed from: the identity of every unary column (what pgx_pearl_unary computed it from, byte for byte),
// the quantised lambda and label cost, the number of sites and the graph.
struct ExpansionBasis {
    std::vector<std::string> ident;
    int64_t lq = 0, hq = 0, n = 0, graph_version = -1;
    bool same_weights_and_graph(const ExpansionBasis& o) const   // (without a pairwise term the graph is not looked at)
    {
        return lq == o.lq && hq == o.hq && n == o.n && (lq <= 0 || graph_version == o.graph_version);
    }
    int leading_columns_unchanged(const ExpansionBasis& now) const   // the memo's prefix
    {
        if (!same_weights_and_graph(now)) return 0;
        size_t p = 0;
        while (p < ident.size() && p < now.ident.size() && ident[p] == now.ident[p]) ++p;
        return (int)p;
    }
    bool unchanged(const ExpansionBasis& now) const   // the identical call's columns, weights and graph
    {
        return ident.size() == now.ident.size() && (size_t)leading_columns_unchanged(now) == ident.size() && same_weights_and_graph(now);
    }
};

// First-cycle memo of pgx_expansion: PEARL starts every labelling it cannot warm-start from the all-zero labelling
// (PEARL.h:507-508, 541-547), so the first cycle's move alpha sees labels < alpha only and is a deterministic function of the
// unary columns 0..alpha, lambda, h and the graph.  The labels after each first-cycle move are kept (expansion.hip holds the
// snapshots); a later expansion from zeros whose leading unary columns are THE SAME (exact identity of what pgx_pearl_unary
// computed them from) restores the state behind that prefix instead of solving its min-cuts again.  Only for lambda > 0.
struct FirstCycleMemo {
    ExpansionBasis from;            // from.ident[a]: identity of the unary column kept move a was solved with
    std::vector<int64_t> changed;   // sites the move relabelled
    int valid = 0;                  // moves 0 .. valid-1 of the last from-zeros expansion are kept
    int keep_prefix(const ExpansionBasis& now, int L)   // leading moves of this call that the memo holds
    {
        const int same = from.leading_columns_unchanged(now);
        if (valid > same) valid = same;
        return valid < L ? valid : L;
    }
    void begin(const ExpansionBasis& now, int L, int prefix)   // this call records moves prefix .. L-1 behind the kept ones
    {
        from.ident.resize((size_t)L);
        changed.resize((size_t)L, 0);
        valid = prefix;
        from.lq = now.lq; from.hq = now.hq; from.n = now.n; from.graph_version = now.graph_version;
    }
    void record(int a, const std::string& ident, int64_t ch)   // once move a's outcome is known (recorded in order: valid stays a prefix)
    {
        if (valid == a) { from.ident[(size_t)a] = ident; changed[(size_t)a] = ch; valid = a + 1; }
    }
    int64_t replay(int prefix, SkipRule& skip) const   // the leading moves as they went last time: the skip rule's bookkeeping, their label changes
    {
        int64_t total = 0;
        for (int a = 0; a < prefix; ++a) { total += changed[(size_t)a]; skip.record(a, changed[(size_t)a]); }
        return total;
    }
    void forget() { valid = 0; from.n = 0; }
};

// The last pgx_expansion that ended on a FIXED POINT (its final cycle relabelled nothing), with what it was computed from: a call
// with the same columns, weights, graph and the labels it left is the same deterministic computation - one cycle of no-ops, the same
// energy - and is answered from here (expansion.hip expansion_launch).  PEARL ends every run with exactly such a call: the iteration
// that finds "nothing changed" labels once more with the models and the warm start of the one before (PEARL.h:429-467).
struct FixedPoint {
    int valid = 0;
    ExpansionBasis from;
    int64_t energy_q = 0;
    int64_t labels_version = -1;   // ExpansionState::labels_version when the fixed point was recorded
};

struct ExpansionCall {   // one pgx_expansion call on the resident problem
    int L = 0;                    // labels of the resident unary table
    int64_t n = 0, labels_n = 0;  // its sites; length of the resident labelling
    int64_t lq = 0, hq = 0, graph_version = 0;
    int max_cycles = 0;
    bool batched = false;         // move_route.h plan_move(...).batched
    bool snapshots_fit = true;    // the memo's L x n snapshots are within its size cap
};

struct CycleCounts {   // moves of one call by what became of them: solved + skipped_host + skipped_device + restored == L x cycles
    int64_t solved = 0, skipped_host = 0, skipped_device = 0, restored = 0;
    int64_t declined = 0;               // batched moves that came back declined (solved again: counted in `solved` once)
    int64_t batches_after_decline = 0;  // batches opened behind a declined move
};

// Everything pgx_expansion remembers between calls, and the events that change it.  Writers of the labels, the unary table and the
// points call the event; nobody else assigns labels_version, labels_all_zero or last_done.
struct ExpansionState {
    FirstCycleMemo memo;
    FixedPoint last_done;
    ExpansionBasis resident;      // ident: per label, what its unary column was computed from (pgx_pearl_unary); empty = unknown (injected
                                  // table).  The other fields are those of the call in progress (see())
    int64_t labels_version = 0;   // bumped by EVERY writer of the labels (pgx_set_labels, every expansion move, the greedy labelling): the
                                  // identical-call shortcut compares it instead of trusting each writer to clear last_done
    int labels_all_zero = 0;      // the resident labelling is the all-zero one pgx_set_labels uploaded (no move has run since)
    int labels_max = 0;           // largest label pgx_set_labels uploaded or a move may have written (the moves index per-label tables with the labels: checked against L)
    int64_t points_version = 0;   // bumped by pgx_set_points
    int mf_memo = 1;              // PGX_MF_MEMO=0: no first-cycle memo, no identical-call answer (A/B)
    int mf_done_verify = 0;       // PGX_MF_DONE_VERIFY=1: on a shortcut hit run the real verifying cycle and check 0 changes + equal energy
    int64_t memo_hits = 0;        // moves restored from the memo or answered from the fixed point (pgx_expansion_paths[1])

    // ---- events
    void labels_written()   // by a move, the greedy labelling or the caller: not the uploaded zeros, not the labels a fixed point left
    {
        labels_all_zero = 0;
        last_done.valid = 0;
        labels_version += 1;
    }
    void labels_uploaded(int largest)   // pgx_set_labels: the labels are the caller's now
    {
        labels_written();
        labels_max = largest;
        labels_all_zero = largest == 0 ? 1 : 0;
    }
    void unary_injected() { resident.ident.clear(); }   // a table without identity: no first-cycle memo, no identical-call shortcut
    void unary_resident(std::vector<std::string>&& ident) { resident.ident = std::move(ident); }
    void points_changed()   // the memo's snapshots belong to the old point set (their owner releases them), and so does every column
    {
        points_version += 1;
        labels_all_zero = 0;
        memo.forget();
        resident.ident.clear();
    }

    // ---- questions
    const ExpansionBasis& see(const ExpansionCall& c)
    {
        resident.lq = c.lq; resident.hq = c.hq; resident.n = c.n; resident.graph_version = c.graph_version;
        return resident;
    }
    bool ident_known(const ExpansionCall& c) const { return c.L > 0 && (int)resident.ident.size() == c.L && c.labels_n == c.n; }
    // identical call: the labels are those the last expansion left at a fixed point, and columns, weights and graph are what it was
    // computed from => one verifying cycle of no-ops and the same energy, without running it
    bool answers(const ExpansionCall& c)
    {
        return mf_memo && last_done.valid && ident_known(c) && c.max_cycles >= 1 && last_done.from.unchanged(see(c)) &&
               last_done.labels_version == labels_version;
    }
    void answer(const ExpansionCall& c, CycleCounts& cnt, int64_t* energy_q, int* cycles)
    {
        memo_hits += c.L;
        cnt.skipped_host += c.L;   // "moves skipped because the labelling had not changed since that label's last move, which relabelled nothing"
        *energy_q = last_done.energy_q;
        *cycles = 1;
    }
};

// GCO-v3 "standard cycles" loop [U-5] as PEARL drives it (PEARL.h:550-551): cycle over the labels in index order until a whole
// cycle leaves the energy unchanged, at most max_cycles cycles.  The backend supplies what touches the device; every call returns
// 0 or the error that ends the expansion:
//   energy(&e)                                   the energy of the resident labelling
//   move(alpha, declined_by_batch, &changed)     one unbatched move, solved before it returns
//   batch_begin()                                a new batch: its moves are enqueued back to back, one host round trip for all
//   batch_enqueue(alpha, slot, skip_rel, &enq)   enq = false: the move was solved or refused instead of enqueued
//   batch_fetch(slots)                           the results of the batch's slots, synchronised
//   batch_result(slot, alpha, &status, &changed) status 0: solved | 1: declined, the labels untouched, nothing behind it ran |
//                                                2: did not run (the skip rule held on the device, or it sits behind a declined move)
//   cycle_l0(&changed)                           lambda = 0: the whole cycle in closed form
//   reserve_snapshots(prefix)                    room for L snapshots, the kept leading `prefix` carried along
//   snapshot(alpha)                              enqueued right behind move alpha of the first cycle: the labels it left
//   restore(prefix)                              the labels as move prefix-1 left them
//   error(format, alpha)                         the text of a broken promise of the batch protocol
#define PGX_CYCLE_TRY(call) do { const int rc_ = (call); if (rc_ != 0) return rc_; } while (0)

template <class Backend>
int run_expansion(ExpansionState& st, const ExpansionCall& c, Backend& be, CycleCounts& cnt, int64_t* energy_q, int* cycles)
{
    const ExpansionBasis& now = st.see(c);
    const bool ident_known = st.ident_known(c);
    // the memo is usable when this expansion starts from the all-zero labelling on columns of known identity
    const bool memo_on = st.mf_memo && c.lq > 0 && st.labels_all_zero && c.L > 1 && ident_known && c.snapshots_fit;
    st.labels_written();   // (the moves below write the labels)
    int64_t new_e = 0;
    PGX_CYCLE_TRY(be.energy(&new_e));
    int64_t old_e = new_e + 1;
    int done = 0;
    int64_t last_cycle_changed = -1;
    SkipRule skip(c.L);
    int memo_p = 0;   // leading moves restored instead of solved
    if (memo_on) {
        memo_p = st.memo.keep_prefix(now, c.L);
        PGX_CYCLE_TRY(be.reserve_snapshots(memo_p));
        st.memo.begin(now, c.L, memo_p);
    }
    for (int cycle = 1; cycle <= c.max_cycles; ++cycle) {
        if (new_e == old_e) break;
        old_e = new_e;
        int64_t changed_total = 0;
        int alpha0 = 0;
        const bool keep = memo_on && cycle == 1;   // this cycle's moves are recorded
        if (keep && memo_p > 0) {
            changed_total += st.memo.replay(memo_p, skip);
            PGX_CYCLE_TRY(be.restore(memo_p));
            st.memo_hits += memo_p;
            cnt.restored += memo_p;
            alpha0 = memo_p;
        }
        if (c.lq <= 0) {   // no pairwise term: closed-form moves, the whole cycle enqueued at once (one host round trip)
            int64_t ch = 0;
            PGX_CYCLE_TRY(be.cycle_l0(&ch));
            changed_total += ch;
            cnt.solved += c.L;
        } else if (c.batched) {
            // The moves of the cycle are enqueued back to back and resolved together - one host round trip per batch instead of one
            // per move.  A move that declines poisons the rest of its batch on the device (they return untouched); it is solved by the
            // general path and the cycle resumes behind it.  The skip rule is applied on the device for moves behind others of the
            // same batch (their outcome is not known when they are enqueued).
            int alpha = alpha0;
            bool behind_decline = false;
            std::vector<int> batch;
            while (alpha < c.L) {
                batch.clear();
                PGX_CYCLE_TRY(be.batch_begin());
                const int64_t version0 = skip.version;
                for (int a = alpha; a < c.L; ++a) {
                    if (batch.empty() && skip.noop_now(a)) { ++cnt.skipped_host; continue; }   // (known now: nothing is in flight)
                    bool enqueued = false;
                    PGX_CYCLE_TRY(be.batch_enqueue(a, (int)batch.size(), skip.skip_rel(a, version0), &enqueued));
                    if (!enqueued) return be.error("pgx_expansion (internal): a batched move was not enqueued", a);
                    batch.push_back(a);
                    if (keep) PGX_CYCLE_TRY(be.snapshot(a));
                }
                if (batch.empty()) break;
                if (behind_decline) ++cnt.batches_after_decline;
                behind_decline = false;
                PGX_CYCLE_TRY(be.batch_fetch((int)batch.size()));
                int next = c.L;
                for (size_t k = 0; k < batch.size(); ++k) {
                    const int a = batch[k];
                    int status = 0;
                    int64_t ch = 0;
                    PGX_CYCLE_TRY(be.batch_result((int)k, a, &status, &ch));
                    if (status == 2) {   // the device applied the skip rule
                        if (!skip.noop_now(a)) return be.error("pgx_expansion: move %d of a batch did not run", a);
                        ++cnt.skipped_device;
                        continue;
                    }
                    if (status == 1) {   // declined: the general path, then a new batch behind it
                        ++cnt.declined;
                        PGX_CYCLE_TRY(be.move(a, true, &ch));
                        if (keep) PGX_CYCLE_TRY(be.snapshot(a));   // (the snapshot taken behind the declined move holds the untouched labels)
                        next = a + 1;
                        behind_decline = true;
                    }
                    ++cnt.solved;
                    if (keep) st.memo.record(a, now.ident[(size_t)a], ch);
                    changed_total += ch;
                    skip.record(a, ch);
                    if (status == 1) break;
                }
                alpha = next;
            }
        } else {
            for (int alpha = alpha0; alpha < c.L; ++alpha) {
                if (skip.noop_now(alpha)) { ++cnt.skipped_host; continue; }
                int64_t ch = 0;
                PGX_CYCLE_TRY(be.move(alpha, false, &ch));
                ++cnt.solved;
                if (keep) { PGX_CYCLE_TRY(be.snapshot(alpha)); st.memo.record(alpha, now.ident[(size_t)alpha], ch); }
                changed_total += ch;
                skip.record(alpha, ch);
            }
        }
        // a cycle that relabels nothing leaves the energy unchanged by construction: skip the recomputation
        if (changed_total > 0) PGX_CYCLE_TRY(be.energy(&new_e));
        done = cycle;
        last_cycle_changed = changed_total;
    }
    if (ident_known && done >= 1 && last_cycle_changed == 0) {   // a fixed point of the whole cycle (a final cycle that moved ties at equal energy is not)
        st.last_done.valid = 1;
        st.last_done.from = now;
        st.last_done.energy_q = new_e;
        st.last_done.labels_version = st.labels_version;
    }
    *energy_q = new_e;
    *cycles = done;
    return 0;
}

}  // namespace pgx
