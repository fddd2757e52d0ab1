// The statements of the row-streaming product, included by linear_fwd_kernel and by linear_fwd_body (linear_fwd.hpp), the device function that
// linear_fwd_jobs_kernel calls.  The two include this text and neither calls the other: through a call the single kernels' registers move
// (profiles/r31_stream_groups.md).  The includer provides
//   the template parameters TCO, PRO, VEC4, EPI, NCH;
//   the parameters X, W, bias, M, Ci, Co, transpose_w, Y, stat_partial, Y2, pro, slope, Xb, xsplit, Yb, ysplit, addend, drop_counter,
//     drop_seed, drop_threshold, drop_scale, mask_ref, mask_slope, uv  (linear_fwd_kernel's list);
//   sW, the launch's dynamic LDS as a float array: [16*TCO][Cip] (+ [5][Cik] prologue coefficients) (+ the output staging tiles);
//   the macros LF_BX, LF_BY (the workgroup's row and column-slab coordinates) and LF_NBX (the row workgroups of its grid): the launch's
//     own in the kernel, the job's in the body function.  The text never reads the launch's coordinates itself.
// The tunables and the rule PF<NCH> (the next row group's fragments in flight too) are linear_fwd.hpp's, beside the planning helpers.
    static_assert(EPI != EPI_ADD_MASK || (PRO && VEC4), "the masked epilogue is the aligned dX product's");
    static_assert(EPI != EPI_UV || (!PRO && VEC4 && NCH == 1), "the combine prologue is the narrow aligned forward's");
    static_assert(EPI != EPI_BN_ACT || !PRO, "the BatchNorm epilogue is the forward product's");
    constexpr bool UV = EPI == EPI_UV, TWO = PRO || UV;              // TWO: two raw fragments per chunk
    constexpr bool BNA = EPI == EPI_BN_ACT;
    // mask_ref [M, Co] (EPI_ADD_MASK): the saved output of the join in front of this block (this block's own input x)
    // drop_counter (not PRO, one-pointer output): Y = dropout_mask .* (X W^T) * drop_scale with the counter-based mask of
    // common.hpp (element e = row * Co + column) -- the backward of nn.Dropout applied while the gradient of the Linear
    // BEHIND the dropout is written, instead of in a pass of its own over [M, Co].
    // addend [M, Co] (PRO only, one-pointer output): Y = X W^T + addend -- the gradient the other consumer of the block's input
    // sent back, so that autograd's accumulation pass over three [M, Co] tensors never runs.
    // Xb / xsplit: the operand is the column concatenation [X | Xb] split at column xsplit (the fusion layers' torch.cat,
    // never materialised); Yb / ysplit: the output columns >= ysplit go to Yb [M, Co - ysplit] (dX of such a layer).
    // Both splits are multiples of 4.
    const int Cip = ((Ci + 15) / 16) * 16 + 4;
    const int Cik = ((Ci + 15) / 16) * 16;
    float* sPro = sW + 16 * TCO * Cip;
    [[maybe_unused]] float* sTile = sPro + (PRO ? 5 * Cik : 0);          // [4 waves][16][16 TCO + 4] output staging (TCO >= 2)
    if constexpr (PRO) {
        for (int t = threadIdx.x; t < 5 * Cik; t += LF_BLOCK) {
            const int which = t / Cik, k = t - which * Cik;
            sPro[t] = k < Ci ? pro[which * Ci + k] : 0.f;
        }
    }
    const int co_base = LF_BY * 16 * TCO;
    if (!transpose_w && (Ci % 4) == 0) {          // rows of W are contiguous: 16-byte loads
        const int Cip4 = Cip / 4, Ci4 = Ci / 4;
        for (int t = threadIdx.x; t < 16 * TCO * Cip4; t += LF_BLOCK) {
            const int r = t / Cip4, k4 = t - r * Cip4;
            const int co = co_base + r;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (co < Co && k4 < Ci4) v = *reinterpret_cast<const float4*>(W + (int64_t)co * Ci + 4 * k4);
            *reinterpret_cast<float4*>(sW + r * Cip + 4 * k4) = v;
        }
    } else {
        for (int t = threadIdx.x; t < 16 * TCO * Cip; t += LF_BLOCK) {
            const int r = t / Cip, k = t - r * Cip;
            const int co = co_base + r;
            float v = 0.f;
            if (co < Co && k < Ci) v = transpose_w ? W[(int64_t)k * Co + co] : W[(int64_t)co * Ci + k];
            sW[t] = v;
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rr = lane & 15, g = lane >> 4;
    const bool vec = (Ci % 4) == 0;
    float bsel[TCO][4];
#pragma unroll
    for (int t = 0; t < TCO; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int co = co_base + 16 * t + 4 * g + e;
            bsel[t][e] = (bias != nullptr && co < Co) ? bias[co] : 0.f;
        }
    // EPI_BN_ACT: the coefficients of the four channels this lane STORES in pass t (the same in every row group): through the staging
    // tile a lane stores float4 number lane + 64 t of the [16][16 TCO] tile, else its own accumulator columns
    [[maybe_unused]] float4 bna[BNA ? TCO : 1], bnb[BNA ? TCO : 1];
    if constexpr (BNA) {
#pragma unroll
        for (int t = 0; t < TCO; ++t) {
            const int co = TCO >= 2 ? co_base + 4 * ((lane + WAVE * t) % (4 * TCO)) : co_base + 16 * t + 4 * g;
            bna[t] = bnb[t] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (co < Co) {
                bna[t] = *reinterpret_cast<const float4*>(pro + co);
                bnb[t] = *reinterpret_cast<const float4*>(pro + Co + co);
            }
        }
    }
    // out = lrelu(add_rn(fmaf(a, y, b), skip), slope) on four channels
    [[maybe_unused]] auto bn_act4 = [&](float4 y, const float4 a, const float4 b, const float* skp) -> float4 {
        float4 o = make_float4(fmaf(a.x, y.x, b.x), fmaf(a.y, y.y, b.y), fmaf(a.z, y.z, b.z), fmaf(a.w, y.w, b.w));
        if (skp != nullptr) {
            const float4 k = *reinterpret_cast<const float4*>(skp);
            o = make_float4(add_rn(o.x, k.x), add_rn(o.y, k.y), add_rn(o.z, k.z), add_rn(o.w, k.w));
        }
        if (slope != 1.f) {
            o.x = o.x > 0.f ? o.x : slope * o.x;
            o.y = o.y > 0.f ? o.y : slope * o.y;
            o.z = o.z > 0.f ? o.z : slope * o.z;
            o.w = o.w > 0.f ? o.w : slope * o.w;
        }
        return o;
    };
    float s1[TCO][4], s2[TCO][4], sh[TCO][4];
#pragma unroll
    for (int t = 0; t < TCO; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) { s1[t][e] = 0.f; s2[t][e] = 0.f; sh[t][e] = 0.f; }
    bool have_shift = false;
    const int nchunk = (Ci + 15) / 16;

    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    // raw operand fragment(s) of chunk c for row r: X (either layout / the two-pointer form), or (gA, y) with PRO
    auto load_raw = [&](int64_t r, bool rv, int c, float4& xa, float4& xb2) {
        const int k0 = 16 * c + 4 * g;
        xa = zero4;
        xb2 = zero4;
        if (!rv || k0 >= Ci) return;
        if constexpr (PRO) {
            xa = *reinterpret_cast<const float4*>(X + r * Ci + k0);
            xb2 = *reinterpret_cast<const float4*>(Y2 + r * Ci + k0);
        } else if constexpr (UV) {
            xa = *reinterpret_cast<const float4*>(X + r * Ci + k0);
            xb2 = *reinterpret_cast<const float4*>(uv.V + r * Ci + k0);
        } else if (Xb != nullptr) {
            if (k0 < xsplit) xa = *reinterpret_cast<const float4*>(X + r * xsplit + k0);
            else xa = *reinterpret_cast<const float4*>(Xb + r * (Ci - xsplit) + (k0 - xsplit));
        } else if (VEC4 || vec) {
            xa = *reinterpret_cast<const float4*>(X + r * Ci + k0);
        } else if constexpr (!VEC4) {
            const float* xp = X + r * Ci;
            xa.x = xp[k0];
            xa.y = k0 + 1 < Ci ? xp[k0 + 1] : 0.f;
            xa.z = k0 + 2 < Ci ? xp[k0 + 2] : 0.f;
            xa.w = k0 + 3 < Ci ? xp[k0 + 3] : 0.f;
        }
    };
    // the MFMA operand of chunk c: the raw fragment, or gY formed from (gA, y) and the staged coefficients
    auto operand = [&](bool rv, int c, float4 gv, float4 yv) -> float4 {
        if constexpr (PRO) {
            const int k0 = 16 * c + 4 * g;
            float4 xv = zero4;
            if (rv && k0 < Ci) {
                const float4 pa = *reinterpret_cast<const float4*>(sPro + k0), pb = *reinterpret_cast<const float4*>(sPro + Cik + k0);
                const float4 al = *reinterpret_cast<const float4*>(sPro + 2 * Cik + k0), be = *reinterpret_cast<const float4*>(sPro + 3 * Cik + k0);
                const float4 de = *reinterpret_cast<const float4*>(sPro + 4 * Cik + k0);
                xv.x = fmaf(al.x * (fmaf(pa.x, yv.x, pb.x) > 0.f ? 1.f : slope), gv.x, fmaf(be.x, yv.x, de.x));
                xv.y = fmaf(al.y * (fmaf(pa.y, yv.y, pb.y) > 0.f ? 1.f : slope), gv.y, fmaf(be.y, yv.y, de.y));
                xv.z = fmaf(al.z * (fmaf(pa.z, yv.z, pb.z) > 0.f ? 1.f : slope), gv.z, fmaf(be.z, yv.z, de.z));
                xv.w = fmaf(al.w * (fmaf(pa.w, yv.w, pb.w) > 0.f ? 1.f : slope), gv.w, fmaf(be.w, yv.w, de.w));
            }
            return xv;
        } else {
            return gv;
        }
    };
    // EPI_UV: this lane's four channels 4 g .. 4 g + 3 are the same in every row group (one chunk): coefficients in registers
    [[maybe_unused]] float4 uva = zero4, uvt = zero4;
    if constexpr (UV) {
        if (LF_BX == 0 && LF_BY == 0 && (int)threadIdx.x < Ci) {
            const UvCoef k = uv_coef(threadIdx.x, Ci, uv.stats, uv.shift, uv.gamma, uv.beta, uv.n_edges, uv.eps);
            uv_publish(threadIdx.x, Ci, k, uv.n_edges, uv.run_mean, uv.run_var, uv.momentum, uv.a2, uv.b2, uv.aux2);
        }
        if (4 * g < Ci) {
            float a[4], tv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const UvCoef k = uv_coef(4 * g + e, Ci, uv.stats, uv.shift, uv.gamma, uv.beta, uv.n_edges, uv.eps);
                a[e] = k.a;
                tv[e] = uv_vcoef(k);
            }
            uva = make_float4(a[0], a[1], a[2], a[3]);
            uvt = make_float4(tv[0], tv[1], tv[2], tv[3]);
        }
    }
    // the MFMA operand out = helper(U, V) of row r, stored on the way by the first column group (rows / channels past the end stay zero)
    [[maybe_unused]] auto uv_operand = [&](int64_t r, bool rv, float4 u, float4 v) -> float4 {
        if (!rv || 4 * g >= Ci) return zero4;
        const float4 o = uv_out4(uva, uvt, u, v);
        if (LF_BY == 0) *reinterpret_cast<float4*>(uv.out + r * Ci + 4 * g) = o;
        return o;
    };
    // (Issuing the operand loads of four row groups in one burst, or prefetching the next group, measured no faster: the
    // write-heavy shapes run at the ~2.7 TB/s HBM WRITE rate -- 163840 x 8 -> 32 moves 21 MB out in 13 us -- not at a
    // per-wavefront latency limit.)
    constexpr int NCA = NCH > 0 ? NCH : 1;
    const int64_t row_stride = (int64_t)LF_NBX * (LF_BLOCK / WAVE) * 16;
    [[maybe_unused]] float4 fa[NCA], fb[TWO ? NCA : 1], na[PF<NCH> ? NCA : 1], nb[(PF<NCH> && TWO) ? NCA : 1];
    [[maybe_unused]] auto load_group = [&](int64_t rw0, float4 (&xa)[NCA], float4 (&xb)[TWO ? NCA : 1]) {
        const int64_t rq = rw0 + rr;
        const bool ok = rw0 < M && rq < M;
#pragma unroll
        for (int c = 0; c < NCA; ++c) {
            float4 t0, t1;
            load_raw(rq, ok, c, t0, t1);
            xa[c] = t0;
            if constexpr (TWO) xb[c] = t1;
        }
    };
    if constexpr (PF<NCH>) load_group(((int64_t)LF_BX * (LF_BLOCK / WAVE) + wave) * 16, fa, fb);
    for (int64_t row0 = ((int64_t)LF_BX * (LF_BLOCK / WAVE) + wave) * 16; row0 < M; row0 += row_stride) {
        const int64_t r = row0 + rr;
        const bool rv = r < M;
        f32x4 acc[TCO];
#pragma unroll
        for (int t = 0; t < TCO; ++t) acc[t] = f32x4{bsel[t][0], bsel[t][1], bsel[t][2], bsel[t][3]};
        if constexpr (NCH > 0) {
            if constexpr (PF<NCH>) {
                if constexpr (TWO) load_group(row0 + row_stride, na, nb);
                else load_group(row0 + row_stride, na, fb);
            } else {
                load_group(row0, fa, fb);
            }
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const int k0 = 16 * c + 4 * g;
                float4 xv;
                if constexpr (UV) xv = uv_operand(r, rv, fa[c], fb[c]);
                else xv = operand(rv, c, fa[c], fb[PRO ? c : 0]);
#pragma unroll
                for (int t = 0; t < TCO; ++t) {
                    const float4 wv = *reinterpret_cast<const float4*>(sW + (16 * t + rr) * Cip + k0);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.x, xv.x, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.y, xv.y, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.z, xv.z, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.w, xv.w, acc[t], 0, 0, 0);
                }
            }
            if constexpr (PF<NCH>) {
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    fa[c] = na[c];
                    if constexpr (TWO) fb[c] = nb[c];
                }
            }
        } else {
        for (int c = 0; c < nchunk; ++c) {
            const int k0 = 16 * c + 4 * g;
            float4 ra, rb;
            load_raw(r, rv, c, ra, rb);
            const float4 xv = operand(rv, c, ra, rb);
#pragma unroll
            for (int t = 0; t < TCO; ++t) {
                const float4 wv = *reinterpret_cast<const float4*>(sW + (16 * t + rr) * Cip + k0);
                // D[i = co][j = row]: A = W fragment (i = lane & 15), B = X fragment (j = lane & 15)
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.x, xv.x, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.y, xv.y, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.z, xv.z, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.w, xv.w, acc[t], 0, 0, 0);
            }
        }
        }
        // lane holds Y[row = row0 + rr][co = co_base + 16 t + 4 g + e], e = 0..3
        if constexpr (TCO >= 2) {
            // Stored straight from the accumulators every store instruction writes 64 bytes into each of 16 rows (measured
            // 1.5-1.7 TB/s on write-heavy shapes); through a per-wave LDS tile [16 rows][16 TCO] every instruction writes
            // whole 128 / 256-byte row segments, consecutive lanes consecutive addresses.
            constexpr int TW = 16 * TCO, TLD = TW + 4, F4R = TW / 4;       // tile width, padded row, float4 per row
            float* tile = sTile + wave * 16 * TLD;
#pragma unroll
            for (int t = 0; t < TCO; ++t)
                *reinterpret_cast<float4*>(tile + rr * TLD + 16 * t + 4 * g) = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
            __builtin_amdgcn_wave_barrier();               // LDS operations of one wave complete in order
#pragma unroll
            for (int i = 0; i < (16 * F4R) / WAVE; ++i) {
                const int qd = lane + WAVE * i, trow = qd / F4R, tc4 = qd - trow * F4R;
                const int64_t orow = row0 + trow;
                const int co = co_base + 4 * tc4;
                if (orow < M && co < Co) {
                    float4 o4 = *reinterpret_cast<const float4*>(tile + trow * TLD + 4 * tc4);
                    if constexpr (EPI == EPI_ADD) {
                        {
                            if (VEC4 || (Co % 4) == 0) {
                                const float4 a4 = *reinterpret_cast<const float4*>(addend + orow * Co + co);
                                o4.x += a4.x; o4.y += a4.y; o4.z += a4.z; o4.w += a4.w;
                            } else {
                                o4.x += addend[orow * Co + co];
                                if (co + 1 < Co) o4.y += addend[orow * Co + co + 1];
                                if (co + 2 < Co) o4.z += addend[orow * Co + co + 2];
                                if (co + 3 < Co) o4.w += addend[orow * Co + co + 3];
                            }
                        }
                    }
                    if constexpr (EPI == EPI_ADD_MASK) {
                        const float4 a4 = *reinterpret_cast<const float4*>(addend + orow * Co + co);
                        const float4 r4 = *reinterpret_cast<const float4*>(mask_ref + orow * Co + co);
                        o4.x += a4.x; o4.y += a4.y; o4.z += a4.z; o4.w += a4.w;
                        o4.x = r4.x > 0.f ? o4.x : mask_slope * o4.x;
                        o4.y = r4.y > 0.f ? o4.y : mask_slope * o4.y;
                        o4.z = r4.z > 0.f ? o4.z : mask_slope * o4.z;
                        o4.w = r4.w > 0.f ? o4.w : mask_slope * o4.w;
                    }
                    if constexpr (BNA) o4 = bn_act4(o4, bna[i], bnb[i], addend != nullptr ? addend + orow * Co + co : nullptr);
                    if constexpr (EPI == EPI_DROPOUT) {
                        {
                            const unsigned long long ctr = (unsigned long long)drop_counter[0];
                            const unsigned long long e = (unsigned long long)(orow * Co + co);
                            o4.x = dropout_keep(drop_seed, ctr, e, drop_threshold) ? o4.x * drop_scale : 0.f;
                            o4.y = dropout_keep(drop_seed, ctr, e + 1, drop_threshold) ? o4.y * drop_scale : 0.f;
                            o4.z = dropout_keep(drop_seed, ctr, e + 2, drop_threshold) ? o4.z * drop_scale : 0.f;
                            o4.w = dropout_keep(drop_seed, ctr, e + 3, drop_threshold) ? o4.w * drop_scale : 0.f;
                        }
                    }
                    if (Yb != nullptr) {
                        if (co < ysplit) *reinterpret_cast<float4*>(Y + orow * ysplit + co) = o4;
                        else *reinterpret_cast<float4*>(Yb + orow * (Co - ysplit) + (co - ysplit)) = o4;
                    } else if (VEC4 || (Co % 4) == 0) {
                        *reinterpret_cast<float4*>(Y + orow * Co + co) = o4;
                    } else if constexpr (!VEC4) {
                        const float ov[4] = {o4.x, o4.y, o4.z, o4.w};
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (co + e < Co) Y[orow * Co + co + e] = ov[e];
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();               // the tile is rewritten by the next row group
        } else {
#pragma unroll
        for (int t = 0; t < TCO; ++t) {
            const int co = co_base + 16 * t + 4 * g;
            if constexpr (EPI == EPI_ADD) {
                if (rv) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (co + e < Co) acc[t][e] += addend[r * Co + co + e];
                }
            }
            if constexpr (EPI == EPI_ADD_MASK) {
                if (rv && co < Co) {
                    const float4 a4 = *reinterpret_cast<const float4*>(addend + r * Co + co);
                    const float4 r4 = *reinterpret_cast<const float4*>(mask_ref + r * Co + co);
                    const float av[4] = {a4.x, a4.y, a4.z, a4.w}, rf[4] = {r4.x, r4.y, r4.z, r4.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float v = acc[t][e] + av[e];
                        acc[t][e] = rf[e] > 0.f ? v : mask_slope * v;
                    }
                }
            }
            if constexpr (BNA) {
                if (rv && co < Co) {
                    const float4 o4 = bn_act4(make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]), bna[t], bnb[t],
                                              addend != nullptr ? addend + r * Co + co : nullptr);
                    acc[t] = f32x4{o4.x, o4.y, o4.z, o4.w};
                }
            }
            if constexpr (EPI == EPI_DROPOUT) {
                if (rv) {
                    const unsigned long long ctr = (unsigned long long)drop_counter[0];
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (co + e < Co)
                            acc[t][e] = dropout_keep(drop_seed, ctr, (unsigned long long)(r * Co + co + e), drop_threshold)
                                            ? acc[t][e] * drop_scale : 0.f;
                }
            }
            if (rv) {
                if (Yb != nullptr) {
                    const float4 o4 = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
                    if (co < ysplit) *reinterpret_cast<float4*>(Y + r * ysplit + co) = o4;
                    else if (co < Co) *reinterpret_cast<float4*>(Yb + r * (Co - ysplit) + (co - ysplit)) = o4;
                } else if (VEC4) {
                    if (co < Co) *reinterpret_cast<float4*>(Y + r * Co + co) = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
                } else if (co + 3 < Co && (Co % 4) == 0) {
                    *reinterpret_cast<float4*>(Y + r * Co + co) = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
                } else if constexpr (!VEC4) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (co + e < Co) Y[r * Co + co + e] = acc[t][e];
                }
            }
        }
        }
        if (!BNA && stat_partial != nullptr) {
            if (!have_shift) {   // shift = this wave's first row (lane with rr == 0 of each co group)
#pragma unroll
                for (int t = 0; t < TCO; ++t)
#pragma unroll
                    for (int e = 0; e < 4; ++e) sh[t][e] = __shfl(acc[t][e], 16 * g, WAVE);
                have_shift = true;
            }
            if (rv) {
#pragma unroll
                for (int t = 0; t < TCO; ++t)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float dlt = acc[t][e] - sh[t][e];
                        s1[t][e] += dlt;
                        s2[t][e] = fmaf(dlt, dlt, s2[t][e]);
                    }
            }
        }
    }
    if (!BNA && stat_partial != nullptr) {
        // one record {shift, n, sum, sumsq} per BLOCK and channel: the 16 row-lanes fold by shuffles, the 4 waves
        // through LDS, re-based on wave 0's shift (sum (v - s0) = a + n d, sum (v - s0)^2 = b + 2 d a + n d^2)
        __syncthreads();                                 // sW is dead: reuse it as [4 waves][4][16*TCO]
        float* sw = sW + wave * 4 * 16 * TCO;
        // rows this wave actually accumulated
        int64_t nrows = 0;
        for (int64_t row0 = ((int64_t)LF_BX * (LF_BLOCK / WAVE) + wave) * 16; row0 < M;
             row0 += (int64_t)LF_NBX * (LF_BLOCK / WAVE) * 16)
            nrows += (M - row0) < 16 ? (M - row0) : 16;
#pragma unroll
        for (int t = 0; t < TCO; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float a = s1[t][e], b = s2[t][e];
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) {
                    a += __shfl_xor(a, o, WAVE);
                    b += __shfl_xor(b, o, WAVE);
                }
                if (rr == 0) {
                    const int cl = 16 * t + 4 * g + e;
                    sw[cl] = sh[t][e];
                    sw[16 * TCO + cl] = (float)nrows;
                    sw[2 * 16 * TCO + cl] = a;
                    sw[3 * 16 * TCO + cl] = b;
                }
            }
        __syncthreads();
        for (int cl = threadIdx.x; cl < 16 * TCO; cl += LF_BLOCK) {
            const int co = co_base + cl;
            if (co >= Co) continue;
            const float s0 = sW[cl];
            double n = 0.0, S1 = 0.0, S2 = 0.0;
            for (int w = 0; w < LF_BLOCK / WAVE; ++w) {
                const float* q = sW + w * 4 * 16 * TCO;
                const double nb = q[16 * TCO + cl];
                if (nb <= 0.0) continue;
                const double d = (double)q[cl] - (double)s0, a = q[2 * 16 * TCO + cl], b = q[3 * 16 * TCO + cl];
                n += nb;
                S1 += a + nb * d;
                S2 += b + 2.0 * d * a + nb * d * d;
            }
            // record layout [block][channel][4]: one aligned 16-byte tuple per (block, channel)
            *reinterpret_cast<float4*>(stat_partial + ((int64_t)LF_BX * Co + co) * 4) =
                make_float4(s0, (float)n, (float)S1, (float)S2);
        }
    }
