// expansion.hip — pgx_expansion on the device: the backend of expansion_cycle.h's cycle driver (what a move, a batch, a snapshot
// and the energy are on the stream), the first-cycle memo's snapshot buffer and the identical-call answer.
// Which moves run, in which schedule, is decided in the header - nothing here looks at the skip rule or the memo's prefix.
#include <vector>

#include "pgx_internal.h"

namespace pgx {

namespace {

constexpr size_t kMemoMaxBytes = (size_t)2 << 30;   // L x n snapshots beyond this: no first-cycle memo

struct DeviceCycle {
    pgx_ctx* ctx;
    int64_t lq, hq;
    size_t row_bytes() const { return (size_t)ctx->dq_n * 4; }
    MoveRequest request(int alpha) const { MoveRequest rq; rq.lambda_q = lq; rq.h_q = hq; rq.alpha = alpha; return rq; }

    int energy(int64_t* e) { return energy_launch(ctx, lq, hq, e); }
    int move(int alpha, bool declined_by_batch, int64_t* changed)
    {
        MoveRequest rq = request(alpha);
        rq.region_declined = declined_by_batch;
        PGX_TRY(expand_alpha_launch(ctx, rq));
        *changed = rq.changed;
        return PGX_OK;
    }
    // (The planner does not look at L: a table of more labels than a move takes opens a batch, and the batch's first expand_alpha_launch
    //  refuses it with the message of an unbatched move - the batch's state is reset by the next region_batch_begin.)
    int batch_begin() { return region_batch_begin(ctx); }
    int batch_enqueue(int alpha, int slot, int skip_rel, bool* enqueued)
    {
        MoveRequest rq = request(alpha);
        rq.batch_slot = slot;
        rq.skip_rel = skip_rel;
        PGX_TRY(expand_alpha_launch(ctx, rq));
        *enqueued = rq.outcome == MoveOutcome::Pending;
        return PGX_OK;
    }
    int batch_fetch(int slots)
    {
        PGX_TRY(region_batch_fetch(ctx, slots));
        PGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return PGX_OK;
    }
    int batch_result(int slot, int alpha, int* status, int64_t* changed) { return region_result(ctx, slot, alpha, status, changed); }
    int cycle_l0(int64_t* changed)
    {
        const size_t L = (size_t)(ctx->L > 0 ? ctx->L : 1);
        std::vector<int64_t> ch(L, 0);
        std::vector<int> ev(L, 0);
        PGX_TRY(expand_cycle_l0(ctx, hq, ch.data(), ev.data()));
        for (int alpha = 0; alpha < ctx->L; ++alpha) *changed += ch[(size_t)alpha];
        return PGX_OK;
    }
    int reserve_snapshots(int prefix)   // room for this call's snapshots (the kept prefix moves along)
    {
        pgx_ctx::MemoSnapshots& s = ctx->memo_snaps;
        if (s.rows >= ctx->L && s.n == ctx->dq_n) return PGX_OK;
        DevBuf grown;
        PGX_TRY(ensure(ctx, grown, (size_t)ctx->L * row_bytes()));
        if (prefix > 0)
            PGX_HIP(ctx, hipMemcpyAsync(grown.p, s.buf.p, (size_t)prefix * row_bytes(), hipMemcpyDeviceToDevice, ctx->stream));
        PGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        release(s.buf);
        s.buf = grown;
        s.rows = ctx->L;
        s.n = ctx->dq_n;
        return PGX_OK;
    }
    int snapshot(int alpha)
    {
        PGX_HIP(ctx, hipMemcpyAsync((char*)ctx->memo_snaps.buf.p + (size_t)alpha * row_bytes(), ctx->labels.p, row_bytes(), hipMemcpyDeviceToDevice, ctx->stream));
        return PGX_OK;
    }
    int restore(int prefix)
    {
        // The restored labelling holds what moves 0 .. prefix-1 wrote last time.  Those moves do not run now, so nothing else tells
        // labels_max: with the whole first cycle restored and max_cycles = 1 it stayed at the uploaded zeros' 0, and a later, smaller
        // table passed the range check with labels up to prefix-1 resident (found by tests/soak_sequences.py, history "from zeros again").
        if (prefix - 1 > ctx->expansion.labels_max) ctx->expansion.labels_max = prefix - 1;
        PGX_HIP(ctx, hipMemcpyAsync(ctx->labels.p, (char*)ctx->memo_snaps.buf.p + (size_t)(prefix - 1) * row_bytes(), row_bytes(), hipMemcpyDeviceToDevice, ctx->stream));
        return PGX_OK;
    }
    int error(const char* format, int alpha) { return fail(ctx, PGX_ERR_INVALID, format, alpha); }
};

}  // namespace

int expansion_launch(pgx_ctx* ctx, int64_t lq, int64_t hq, int max_cycles, bool allow_shortcut, int64_t* energy_q, int* cycles)
{
    for (int k = 0; k < 8; ++k) ctx->stats[k] = 0;
    ExpansionState& st = ctx->expansion;
    ExpansionCall c;
    c.L = ctx->L; c.n = ctx->dq_n; c.labels_n = ctx->labels_n;
    c.lq = lq; c.hq = hq; c.graph_version = ctx->graph_version;
    c.max_cycles = max_cycles;
    c.batched = plan_move(ctx->route, ctx->dq_n, ctx->max_degree, ctx->gn, MoveKind::Cycle, false).batched;
    c.snapshots_fit = (size_t)(ctx->L > 0 ? ctx->L : 0) * (size_t)ctx->dq_n * 4 <= kMemoMaxBytes;
    CycleCounts cnt;
    if (allow_shortcut && st.answers(c)) {
        if (st.labels_max >= ctx->L) return fail(ctx, PGX_ERR_INVALID, "pgx_expansion: label %d out of range (the unary table has %d labels)", st.labels_max, ctx->L);
        st.answer(c, cnt, energy_q, cycles);
        ctx->stats[7] += cnt.skipped_host;
        if (st.mf_done_verify) {   // debug mode: run the cycle the shortcut stands for and insist on what it promises (its statistics stay)
            int64_t eq2 = 0;
            int cyc2 = 0;
            PGX_TRY(expansion_launch(ctx, lq, hq, max_cycles, false, &eq2, &cyc2));
            if (eq2 != *energy_q || cyc2 != 1 || ctx->stats[4] != 0)
                return fail(ctx, PGX_ERR_INVALID, "pgx_expansion (PGX_MF_DONE_VERIFY): the identical-call shortcut would have answered energy %lld, 1 cycle, 0 changes; "
                                                  "the real cycle gave energy %lld, %d cycle(s), %lld change(s)", (long long)*energy_q, (long long)eq2, cyc2, (long long)ctx->stats[4]);
        }
        return PGX_OK;
    }
    DeviceCycle be{ctx, lq, hq};
    const int rc = run_expansion(st, c, be, cnt, energy_q, cycles);
    ctx->stats[7] += cnt.skipped_host + cnt.skipped_device;
    if (rc != PGX_OK) (void)hipStreamSynchronize(ctx->stream);   // (moves of an abandoned batch may still be in flight)
    return rc;
}

void expansion_points_changed(pgx_ctx* ctx)
{
    ctx->expansion.points_changed();
    pgx_ctx::MemoSnapshots& s = ctx->memo_snaps;
    if (s.buf.p) { (void)hipStreamSynchronize(ctx->stream); release(s.buf); }   // first-cycle snapshots of the old point set
    s.rows = 0;
    s.n = 0;
}

}  // namespace pgx
