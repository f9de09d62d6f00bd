// ott_exact_finish_stage.inc — one stage of a queued row out of the wave's stage buffer into the row's eight chains and its remainder
// sum: the full sweep's additions in its order.  Included by both finishes of the pruned sweep's deferred-tail queue (ott_exact.hip:
// pq_finish, pq_finish_few), so that they share one copy of the arithmetic.  The including scope provides
//   cs_stage  the stage (uint32_t),  cs_row  the lane's 32 floats of it in the stage buffer (const float*),
//   cs_swz    the XOR swizzle of the row's 16-B slots (int),  acc[8], tail  the row's sums.
#pragma unroll
for (int j = 0; j < KC / 8; j++) {
    const uint32_t col = cs_stage * KC + 8 * j;
    if (col < p.dim) {
        const float4 a = *reinterpret_cast<const float4*>(cs_row + (((2 * j) ^ cs_swz) << 2));
        const float4 b = *reinterpret_cast<const float4*>(cs_row + (((2 * j + 1) ^ cs_swz) << 2));
        const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        if (col + 8 <= p.dim) {
#pragma unroll
            for (int l = 0; l < 8; l++) acc[l] = __fadd_rn(acc[l], exact_term<MK>(Q[col + l], x[l]));
        } else {
            const uint32_t nt = p.dim - col;
#pragma unroll
            for (int l = 0; l < 7; l++)
                if ((uint32_t)l < nt) tail = __fadd_rn(tail, exact_term<MK>(Q[col + l], x[l]));
        }
    }
}
