// The statements of pass 1 of the fused MLP backward, included by mlp_bwd_p1_kernel and by mlp_bwd_p1_body (mlp_bwd.hip), the device function
// that mlp_bwd_p1_jobs_kernel calls.  The two include this text and neither calls the other: through a call the single kernel's registers
// move (profiles/r31_stream_groups.md).  The includer provides
//   the template parameters TCO, TCI;
//   the parameters GA, Y, X, X2, split, coef, slope, M, Co, Ci, rows_per_block, PA, PB, PG, PX, ticket, dgamma, dbeta, bcoef
//     (mlp_bwd_p1_kernel's list);
//   the LDS: s_red [WG_WAVES][TCO TCI 256] floats, 16-byte aligned; s_v [WG_WAVES][(2 TCO + TCI) 16] floats; s_own, 5 WG_BLOCK doubles
//     (read only where !P1_ALIAS<TCO, TCI>); s_flag, one int;
//   the macros P1_BX, P1_BY, P1_BZ (the workgroup's coordinates), P1_NBX (the row slices of its grid) and P1_LAST (whether this workgroup is
//     the last of its grid to arrive at `ticket`): the launch's own in the kernel, the job's in the body function.  The text never reads the
//     launch's coordinates itself.
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int co_base = P1_BY * 16 * TCO, ci_base = P1_BZ * 16 * TCI;
    const int kk = lane >> 4, cc = lane & 15;
    f32x4 accA[TCO][TCI], accB[TCO][TCI];
#pragma unroll
    for (int a = 0; a < TCO; ++a)
#pragma unroll
        for (int b = 0; b < TCI; ++b) { accA[a][b] = f32x4{0.f, 0.f, 0.f, 0.f}; accB[a][b] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    float ca[TCO], cb[TCO], cm[TCO], cr[TCO], sg[TCO], sgy[TCO], sx[TCI];
#pragma unroll
    for (int a = 0; a < TCO; ++a) {
        const int co = co_base + 16 * a + cc;
        const bool ok = co < Co;
        ca[a] = ok ? coef[co] : 0.f;
        cb[a] = ok ? coef[Co + co] : 0.f;
        cm[a] = ok ? coef[2 * Co + co] : 0.f;
        cr[a] = ok ? coef[3 * Co + co] : 0.f;
        sg[a] = 0.f;
        sgy[a] = 0.f;
    }
#pragma unroll
    for (int b = 0; b < TCI; ++b) sx[b] = 0.f;

    const int64_t row_begin = (int64_t)P1_BX * rows_per_block;
    const int64_t row_end = row_begin + rows_per_block < M ? row_begin + rows_per_block : M;
#ifndef P1_PREFETCH_
#define P1_PREFETCH_ 0
#endif
    struct Frag { float gv[4][TCO], yv[4][TCO], bv[4][TCI]; };
    auto load = [&](int64_t r0, Frag& f) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t r = r0 + 4 * u + kk;
            const bool rv = r < row_end;
#pragma unroll
            for (int a = 0; a < TCO; ++a) {
                const int co = co_base + 16 * a + cc;
                const bool ok = rv && co < Co;
                f.gv[u][a] = ok ? GA[r * Co + co] : 0.f;
                f.yv[u][a] = ok ? Y[r * Co + co] : cm[a];          // yh = 0 on padding
            }
#pragma unroll
            for (int b = 0; b < TCI; ++b) {
                const int ci = ci_base + 16 * b + cc;
                float xv = 0.f;
                if (rv && ci < Ci) xv = (X2 == nullptr || ci < split) ? X[r * (X2 ? split : Ci) + ci] : X2[r * (Ci - split) + (ci - split)];
                f.bv[u][b] = xv;
            }
        }
    };
    auto compute = [&](const Frag& f) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int b = 0; b < TCI; ++b) sx[b] += f.bv[u][b];
#pragma unroll
            for (int a = 0; a < TCO; ++a) {
                const float g1 = f.gv[u][a] * (fmaf(ca[a], f.yv[u][a], cb[a]) > 0.f ? 1.f : slope);
                const float yh = (f.yv[u][a] - cm[a]) * cr[a];
                sg[a] += g1;
                sgy[a] = fmaf(g1, yh, sgy[a]);
#pragma unroll
                for (int b = 0; b < TCI; ++b) {
                    accA[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(g1, f.bv[u][b], accA[a][b], 0, 0, 0);
                    accB[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(yh, f.bv[u][b], accB[a][b], 0, 0, 0);
                }
            }
        }
    };
    if constexpr (P1_PREFETCH_ != 0) {
        // the next 16-row group's fragments are requested before this group's products (rows past the slice load nothing)
        Frag cur, nxt;
        load(row_begin + 16 * wave, cur);
        for (int64_t r0 = row_begin + 16 * wave; r0 < row_end; r0 += 16 * WG_WAVES) {
            load(r0 + 16 * WG_WAVES, nxt);
            compute(cur);
            cur = nxt;
        }
    } else {
        for (int64_t r0 = row_begin + 16 * wave; r0 < row_end; r0 += 16 * WG_WAVES) {
            Frag f;
            load(r0, f);
            compute(f);
        }
    }
    // C/D layout of 16x16x4: col = lane & 15 (j = ci), row = 4 * (lane >> 4) + reg (i = co)
    const int64_t pb = (int64_t)P1_BX;
    for (int pass = 0; pass < 2; ++pass) {
        if (pass) __syncthreads();
#pragma unroll
        for (int a = 0; a < TCO; ++a)
#pragma unroll
            for (int b = 0; b < TCI; ++b)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    s_red[wave][(a * TCI + b) * 256 + (4 * kk + g) * 16 + cc] = pass ? accB[a][b][g] : accA[a][b][g];
        if (pass == 0) {
            // per-channel sums: lanes with the same cc over the 4 k-groups
#pragma unroll
            for (int a = 0; a < TCO; ++a) {
                float t1 = sg[a], t2 = sgy[a];
                t1 += __shfl_xor(t1, 16, WAVE); t1 += __shfl_xor(t1, 32, WAVE);
                t2 += __shfl_xor(t2, 16, WAVE); t2 += __shfl_xor(t2, 32, WAVE);
                if (kk == 0) { s_v[wave][a * 16 + cc] = t1; s_v[wave][(TCO + a) * 16 + cc] = t2; }
            }
#pragma unroll
            for (int b = 0; b < TCI; ++b) {
                float t1 = sx[b];
                t1 += __shfl_xor(t1, 16, WAVE); t1 += __shfl_xor(t1, 32, WAVE);
                if (kk == 0) s_v[wave][(2 * TCO + b) * 16 + cc] = t1;
            }
        }
        __syncthreads();
        float* dst = pass ? PB : PA;
        for (int t = threadIdx.x; t < TCO * TCI * 256; t += WG_BLOCK) {
            float v = 0.f;
#pragma unroll
            for (int w = 0; w < WG_WAVES; ++w) v += s_red[w][t];
            const int tile = t >> 8, a = tile / TCI, b = tile % TCI, i = (t >> 4) & 15, j = t & 15;
            const int co = co_base + 16 * a + i, ci = ci_base + 16 * b + j;
            if (co < Co && ci < Ci) dst[(pb * Co + co) * Ci + ci] = v;
        }
    }
    const __amdgpu_buffer_rsrc_t pgr = make_rsrc(PG, (int)P1_NBX * 2 * Co * 4);
    for (int t = threadIdx.x; t < (2 * TCO + TCI) * 16; t += WG_BLOCK) {
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < WG_WAVES; ++w) v += s_v[w][t];
        const int grp = t >> 4, c16 = t & 15;
        if (grp < 2 * TCO) {                                   // sum g1 | sum g1 yh: slabs of ci-slab 0 only
            const int which = grp / TCO, co = co_base + 16 * (grp % TCO) + c16;
            if (P1_BZ == 0 && co < Co) st1_sc1(pgr, (((int)pb * 2 + which) * Co + co) * 4, v);   // write-through: summed in this launch
        } else {                                               // column sums of X: slabs of co-slab 0 only
            const int ci = ci_base + 16 * (grp - 2 * TCO) + c16;
            if (P1_BY == 0 && ci < Ci) PX[pb * Ci + ci] = v;
        }
    }
    // The channel part of the finalize (dgamma, dbeta, the coefficients of gY for the dX pass) by the LAST workgroup of this launch
    // to finish (gridsync.hpp): the launch between the two passes of the block's backward disappears.  2 Co <= WG_BLOCK slots.
    if (ticket == nullptr || !P1_LAST) return;
    double* s_buf = P1_ALIAS<TCO, TCI> ? reinterpret_cast<double*>(&s_red[0][0]) : s_own;   // the 10 KB of sums inside s_red where they fit
    double* s_tot = s_buf + 4 * WG_BLOCK;
    sum_partial_rows_f64<WG_BLOCK>(pgr, (int)P1_NBX, 2 * Co, s_buf, s_tot);
    if ((int)threadIdx.x < Co) mlp_channel_part(threadIdx.x, s_tot[threadIdx.x], s_tot[Co + threadIdx.x], coef, M, Co, dgamma, dbeta, bcoef);
