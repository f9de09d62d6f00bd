// ott_maxsim_gather_step.inc — one 32-row step of a workgroup over the rows of one listed group: the body of the `for (base ...)`
// loop of maxsim_gather_kernel (ott_maxsim_gather.hip) and of maxsim_gather_batch_kernel (ott_maxsim_batch.hip), included as TEXT by
// both.  From the mask checks through exact_term, the reduce8 in either order, the remainder, the cosine scaling, the NaN drop and
// ord_of to the running maxima: the additions and their order are exact_gather8_kernel's (ott_exact_dev.h), so the bits are the
// reference's.  Text and not a __device__ function: as a function — by reference, by value, forced inline or not — the same body
// compiled to 206-210 VGPRs at 32 tokens (182-194 as text) and lost a wave of occupancy at 16 (profiles/maxsim_rerank_batch).
// In scope where it is included: MK, NT, NTP (template / constexpr); p (rows, inv, row_mask, row_mask_bits, chunk_mask, chunk_rows,
// gix, ld, metric, reduce); sT, sQi (LDS); start, count, base; wave, lane, grp, c; full, nt; take_max; best[NT].  `continue` leaves
// the step.
            const uint32_t ri = base + 8u * (uint32_t)wave + (uint32_t)grp;
            bool valid = ri < count;
            const uint32_t row = p.gix[start + (valid ? ri : count - 1)];  // a place past the group's end is clamped for the loads, invalid for the maxima
            if (valid && p.row_mask != nullptr && row < p.row_mask_bits) valid = (p.row_mask[row >> 6] >> (row & 63)) & 1;  // src/vec.rs:231-237
            if (valid && p.chunk_mask != nullptr) {
                const uint32_t ch = row / p.chunk_rows;
                valid = (p.chunk_mask[ch >> 6] >> (ch & 63)) & 1;
            }
            if (__ballot(valid) == 0) continue;  // every row of this wave's step is masked: they are never read
            const float* rp = p.rows + (uint64_t)row * p.ld;
            float vinv = 0.0f;
            if (p.metric == OTT_METRIC_COSINE) vinv = p.inv[row];

            // chain c of the row, for every token of the pass: acc = acc + term(q[8j + c], v[8j + c]), j ascending (vec_compute.rs:12-13, 39-42)
            float acc[NT];
#pragma unroll
            for (int q = 0; q < NT; q++) acc[q] = 0.0f;
            auto step = [&](uint32_t jj, float xv) {
                const float4* tq = reinterpret_cast<const float4*>(sT + (size_t)(8 * jj + c) * NTP);
#pragma unroll
                for (int q4 = 0; q4 < NT / 4; q4++) {
                    const float4 t = tq[q4];
                    acc[4 * q4 + 0] = __fadd_rn(acc[4 * q4 + 0], exact_term<MK>(t.x, xv));
                    acc[4 * q4 + 1] = __fadd_rn(acc[4 * q4 + 1], exact_term<MK>(t.y, xv));
                    acc[4 * q4 + 2] = __fadd_rn(acc[4 * q4 + 2], exact_term<MK>(t.z, xv));
                    acc[4 * q4 + 3] = __fadd_rn(acc[4 * q4 + 3], exact_term<MK>(t.w, xv));
                }
            };
            uint32_t j = 0;
            for (; j + MG_UNROLL <= full; j += MG_UNROLL) {
                float x[MG_UNROLL];
#pragma unroll
                for (int u = 0; u < MG_UNROLL; u++) x[u] = rp[8 * (j + u) + c];
#pragma unroll
                for (int u = 0; u < MG_UNROLL; u++) step(j + u, x[u]);
            }
            for (; j < full; j++) step(j, rp[8 * j + c]);
            // remainder: sequential sum of the last dim % 8 terms (vec_compute.rs:15-21, 44-53); every lane of the group computes it
            float tail[NT];
#pragma unroll
            for (int q = 0; q < NT; q++) tail[q] = 0.0f;
            for (uint32_t l = 0; l < nt; l++) {
                const float xv = rp[8 * full + l];
                const float4* tq = reinterpret_cast<const float4*>(sT + (size_t)(8 * full + l) * NTP);
#pragma unroll
                for (int q4 = 0; q4 < NT / 4; q4++) {
                    const float4 t = tq[q4];
                    tail[4 * q4 + 0] = __fadd_rn(tail[4 * q4 + 0], exact_term<MK>(t.x, xv));
                    tail[4 * q4 + 1] = __fadd_rn(tail[4 * q4 + 1], exact_term<MK>(t.y, xv));
                    tail[4 * q4 + 2] = __fadd_rn(tail[4 * q4 + 2], exact_term<MK>(t.z, xv));
                    tail[4 * q4 + 3] = __fadd_rn(tail[4 * q4 + 3], exact_term<MK>(t.w, xv));
                }
            }
#pragma unroll
            for (int q = 0; q < NT; q++) {
                // wide::f32x8::reduce_add across the group's eight lanes (exact_gather8_kernel's)
                float sum;
                if (p.reduce == OTT_REDUCE_SEQ4) {
                    const int b = lane & ~7;
                    float l8[8];
#pragma unroll
                    for (int i = 0; i < 8; i++) l8[i] = __shfl(acc[q], b + i);
                    sum = reduce8(l8, OTT_REDUCE_SEQ4);
                } else {
                    const float s1 = __fadd_rn(acc[q], __shfl_xor(acc[q], 4));  // l_c + l_{c^4}
                    const float s2 = __fadd_rn(s1, __shfl_xor(s1, 2));          // (l0+l4)+(l2+l6) on even-pair lanes, (l1+l5)+(l3+l7) on the others
                    sum = __fadd_rn(s2, __shfl_xor(s2, 1));                     // (a + b == b + a bit for bit)
                }
                float sc = __fadd_rn(sum, tail[q]);
                if (p.metric == OTT_METRIC_COSINE) sc = __fmul_rn(__fmul_rn(sc, sQi[q]), vinv);  // vec_compute.rs:31
                const uint32_t o = (valid && !(sc != sc)) ? ord_of(sc, take_max) : 0u;  // NaN dropped: vec_compute.rs:237
                if (o > best[q]) best[q] = o;
            }
