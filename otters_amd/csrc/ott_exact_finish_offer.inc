// ott_exact_finish_offer.inc — the n queued rows' sums are whole: the score, the filter, the wave's list, and the queue moves on.
// Included behind the stage loop of both finishes of the pruned sweep's deferred-tail queue (ott_exact.hip: pq_finish,
// pq_finish_few).  The including scope provides n, valid, acc[8], tail, vinv and my_row.
float sc = __fadd_rn(reduce8(acc, p.reduce), tail);
if (p.metric == OTT_METRIC_COSINE) sc = __fmul_rn(__fmul_rn(sc, qinv[0]), vinv);
const bool pass = valid && !(sc != sc) && cmp_holds(sc, p.cmp, p.thr);
const uint64_t key = ((uint64_t)ord_of(sc, take_max) << 32) | (uint32_t)(~(my_row + p.tie_off));
if (fresh[0]) {
    wl_fill_sorted(L[0], tk[0], tq[0], p.k, pass, key, p.q0, lane, p.tie_sh);
    fresh[0] = false;
} else if constexpr (!BLK) {
    wl_offer(L[0], tk[0], tq[0], p.k, pass, key, p.q0, lane, p.tie_sh);
} else {
    wl_offer_block(L[0], tk[0], tq[0], p.k, pass, key, p.q0, lane, p.tie_sh);
}
pq_head = (pq_head + n) & (PQ_CAP - 1);
pq_n -= n;
tails_done += n;
