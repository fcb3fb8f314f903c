    // The body of rank_aggregate_kernel (AGG_MODES 0) and of rank_aggregate_modes_kernel (AGG_MODES 1);
    // gp_aggregate.hip includes it once in each, between the kernel's braces. With AGG_MODES 0 the
    // preprocessed text is gp_rank_aggregate's kernel as it was before the hypotheses existed, so its
    // instruction stream does not depend on them; every addition sits under `#if AGG_MODES` and uses the
    // modes kernel's extra argument `ma`.
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    AggSmem& sm = *reinterpret_cast<AggSmem*>(smem_raw);
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* P = poses + (size_t)b * K * 9;
    const float* E = energy + (size_t)b * K * 2;
    // ---- 1. descending ranks, ties by lower index (stable); a total order, so the ranks are a
    //         permutation whatever the energies hold (precedes(): NaN first, as torch.sort orders it)
    for (int i = tid; i < K; i += AGG_THREADS) {
        const float er = E[2 * i], et = E[2 * i + 1];
        int rr = 0, rt = 0;
        for (int j = 0; j < K; ++j) {
            rr += precedes(E[2 * j], j, er, i);
            rt += precedes(E[2 * j + 1], j, et, i);
        }
        sm.rank_rot[i] = rr;
        sm.rank_tr[i] = rt;
    }
    __syncthreads();
    for (int i = tid; i < K; i += AGG_THREADS) {
        if (sm.rank_rot[i] < keep) sm.ord_rot[sm.rank_rot[i]] = i;
        if (sm.rank_tr[i] < keep) sm.ord_tr[sm.rank_tr[i]] = i;
        if (sorted_pose) {  // sorted_poses: rotation part by rotation rank, translation by translation rank
            float* o = sorted_pose + ((size_t)b * K + sm.rank_rot[i]) * 9;
            for (int c = 0; c < 6; ++c) o[c] = P[9 * i + c];
            float* ot = sorted_pose + ((size_t)b * K + sm.rank_tr[i]) * 9;
            for (int c = 6; c < 9; ++c) ot[c] = P[9 * i + c];
        }
        if (sorted_energy) {
            sorted_energy[((size_t)b * K + sm.rank_rot[i]) * 2 + 0] = E[2 * i];
            sorted_energy[((size_t)b * K + sm.rank_tr[i]) * 2 + 1] = E[2 * i + 1];
        }
    }
    __syncthreads();
    // ---- 2./3. quaternions of the kept rotations
    for (int r = tid; r < keep; r += AGG_THREADS) {
        float v[6];
        for (int c = 0; c < 6; ++c) v[c] = P[9 * sm.ord_rot[r] + c];
        float q[4];
        rot6_to_quat(v, q);
        const float sg = q[0] > 0.f ? 1.f : -1.f;   // ((Q[..., 0:1] > 0).float() - 0.5) * 2
        for (int c = 0; c < 4; ++c) {
            sm.q[r][c] = q[c];
            sm.qo[r][c] = sg * q[c];
        }
    }
    __syncthreads();
    if (tid == 0) {
        // average_quaternion_batch with uniform weights: A = sum_r w qo qo^T / sum w
        const float w = 1.0f / (float)keep;
        float wsum = 0.f;
        for (int r = 0; r < keep; ++r) wsum += w;
        double A[4][4];
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) {
                float acc = 0.f;
                for (int r = 0; r < keep; ++r) acc += (sm.qo[r][i] * sm.qo[r][j]) * w;
                A[i][j] = (double)(acc / wsum);
            }
        top_eigvec4(A, sm.qavg);
    }
    // ---- 4. DBSCAN over rows of D = 1 - <qi, qj>^2
    if (clustering) {
        for (int e = tid; e < keep * keep; e += AGG_THREADS) {
            const int i = e / keep, j = e - i * keep;
            const float dot = ((sm.q[i][0] * sm.q[j][0] + sm.q[i][1] * sm.q[j][1]) + sm.q[i][2] * sm.q[j][2]) +
                              sm.q[i][3] * sm.q[j][3];
            sm.D[i][j] = 1.f - dot * dot;
        }
        __syncthreads();
        for (int e = tid; e < keep * keep; e += AGG_THREADS) {
            const int i = e / keep, j = e - i * keep;
            double d2 = 0.0;
            for (int c = 0; c < keep; ++c) {
                const double df = (double)sm.D[i][c] - (double)sm.D[j][c];
                d2 += df * df;
            }
            sm.adj[i][j] = sqrt(d2) <= (double)eps;
        }
        __syncthreads();
        for (int i = tid; i < keep; i += AGG_THREADS) {
            int cnt = 0;
            for (int j = 0; j < keep; ++j) cnt += sm.adj[i][j];
            sm.ncount[i] = cnt;
            sm.label[i] = -1;
        }
        __syncthreads();
        if (tid == 0) {
            // -1 unvisited, -2 queued; membership does not depend on the expansion order
            int nlab = 0;
            for (int i = 0; i < keep; ++i) {
                if (sm.label[i] != -1 || sm.ncount[i] < min_samples) continue;
                int top = 0;
                sm.stack[top++] = i;
                sm.label[i] = -2;
                while (top > 0) {
                    const int p = sm.stack[--top];
                    sm.label[p] = nlab;
                    if (sm.ncount[p] < min_samples) continue;   // border point: not expanded
                    for (int j = 0; j < keep; ++j)
                        if (sm.label[j] == -1 && sm.adj[p][j]) {
                            sm.label[j] = -2;
                            sm.stack[top++] = j;
                        }
                }
                ++nlab;
            }
#if AGG_MODES
            // the counts, the order and the averages of every cluster run on separate lanes below
            reinterpret_cast<ModeSmem*>(smem_raw + sizeof(AggSmem))->nlab = nlab;
#else
            if (nlab > 0) {
                int best = 0, bestc = -1;
                for (int l = 0; l < nlab; ++l) {
                    int c = 0;
                    for (int i = 0; i < keep; ++i) c += sm.label[i] == l;
                    if (c > bestc) { bestc = c; best = l; }
                }
                const float w = 1.0f / (float)bestc;
                float wsum = 0.f;
                for (int r = 0; r < bestc; ++r) wsum += w;
                double A[4][4];
                for (int i = 0; i < 4; ++i)
                    for (int j = 0; j < 4; ++j) {
                        float acc = 0.f;
                        for (int r = 0; r < keep; ++r)
                            if (sm.label[r] == best) acc += (sm.qo[r][i] * sm.qo[r][j]) * w;
                        A[i][j] = (double)(acc / wsum);
                    }
                top_eigvec4(A, sm.qavg);
            }
#endif
        }
    }
#if AGG_MODES
    {
        // ---- 4b. hypotheses: one lane per label for the counts and the order, one lane per slot for the
        //          Jacobi solve and the means (thread 0 above only grew the clusters)
        ModeSmem& ms = *reinterpret_cast<ModeSmem*>(smem_raw + sizeof(AggSmem));
        const int M = ma.max_modes;
        __syncthreads();
        const int L = clustering ? ms.nlab : 0;
        for (int l = tid; l < L; l += AGG_THREADS) {
            int c = 0;
            for (int i = 0; i < keep; ++i) c += sm.label[i] == l;
            ms.lcount[l] = c;
        }
        if (tid == AGG_THREADS - 1) {
            int noise = 0;
            if (clustering)
                for (int i = 0; i < keep; ++i) noise += sm.label[i] == -1;
            ma.n_clusters[b] = L;
            ma.noise_count[b] = noise;
        }
        __syncthreads();
        for (int l = tid; l < L; l += AGG_THREADS) {   // descending count, ties -> lower label (numpy argmax)
            const int c = ms.lcount[l];
            int rk = 0;
            for (int j = 0; j < L; ++j) rk += ms.lcount[j] > c || (ms.lcount[j] == c && j < l);
            if (rk < M) ms.slot_label[rk] = l;
        }
        __syncthreads();
        const int filled = L < 1 ? 1 : (L < M ? L : M);
        if (tid < filled) {
            const int sel = L > 0 ? ms.slot_label[tid] : -1;
            const int cnt = L > 0 ? ms.lcount[sel] : keep;
            float qm[4];
            if (L > 0) {   // the re-average of gp_rank_aggregate, for this slot's label
                const float w = 1.0f / (float)cnt;
                float wsum = 0.f;
                for (int r = 0; r < cnt; ++r) wsum += w;
                double A[4][4];
                for (int i = 0; i < 4; ++i)
                    for (int j = 0; j < 4; ++j) {
                        float acc = 0.f;
                        for (int r = 0; r < keep; ++r)
                            if (sm.label[r] == sel) acc += (sm.qo[r][i] * sm.qo[r][j]) * w;
                        A[i][j] = (double)(acc / wsum);
                    }
                top_eigvec4(A, qm);
                if (tid == 0)   // slot 0 is the largest cluster: the aggregated rotation
                    for (int c = 0; c < 4; ++c) sm.qavg[c] = qm[c];
            } else {   // no cluster: the average of the whole kept set (step 3)
                for (int c = 0; c < 4; ++c) qm[c] = sm.qavg[c];
            }
            float en, spread;
            mode_means(sm, P, E, keep, sel, cnt, qm, ms.mt[tid], &en, &spread);
            for (int c = 0; c < 4; ++c) ms.mq[tid][c] = qm[c];
            ma.mode_count[(size_t)b * M + tid] = cnt;
            ma.mode_energy[(size_t)b * M + tid] = en;
            ma.mode_spread[(size_t)b * M + tid] = spread;
        } else if (tid < M) {
            ma.mode_count[(size_t)b * M + tid] = 0;
            ma.mode_energy[(size_t)b * M + tid] = 0.f;
            ma.mode_spread[(size_t)b * M + tid] = 0.f;
        }
        __syncthreads();
        for (int idx = tid; idx < M * 16; idx += AGG_THREADS) {
            const int m = idx >> 4, r = (idx >> 2) & 3, c = idx & 3;
            float v;
            if (m >= filled) {
                v = 0.f;
            } else if (r == 3) {
                v = c == 3 ? 1.f : 0.f;
            } else if (c == 3) {
                v = ms.mt[m][r];
            } else if (m == 0) {
                continue;   // slot 0's rotation is the aggregated one: step 5 writes the same value to both
            } else {  // quaternion_to_matrix, as in step 5
                const float qr = ms.mq[m][0], qi = ms.mq[m][1], qj = ms.mq[m][2], qk = ms.mq[m][3];
                const float two_s = 2.0f / (((qr * qr + qi * qi) + qj * qj) + qk * qk);
                const float mm[9] = {1 - two_s * (qj * qj + qk * qk), two_s * (qi * qj - qk * qr), two_s * (qi * qk + qj * qr),
                                     two_s * (qi * qj + qk * qr), 1 - two_s * (qi * qi + qk * qk), two_s * (qj * qk - qi * qr),
                                     two_s * (qi * qk - qj * qr), two_s * (qj * qk + qi * qr), 1 - two_s * (qi * qi + qj * qj)};
                v = 0.f;
#pragma unroll
                for (int e = 0; e < 9; ++e)
                    if (e == r * 3 + c) v = mm[e];
            }
            ma.mode_pose[(size_t)b * M * 16 + idx] = v;
        }
        if (tid == 0) {   // the slot nearest to the previous rotation: max <q_m, q_prev>^2, ties -> lower m
            int near = -1;
            if (ma.prev_rot) {
#pragma clang fp contract(off)
                const float* R = ma.prev_rot + (size_t)b * 9;
                const float v6[6] = {R[0], R[3], R[6], R[1], R[4], R[7]};   // columns 0 and 1
                float qp[4];
                rot6_to_quat(v6, qp);
                float bestd = 0.f;
                for (int m = 0; m < filled; ++m) {
                    const float dot = ((ms.mq[m][0] * qp[0] + ms.mq[m][1] * qp[1]) + ms.mq[m][2] * qp[2]) +
                                      ms.mq[m][3] * qp[3];
                    const float d = dot * dot;
                    if (near < 0 || d > bestd) { bestd = d; near = m; }
                }
            }
            ma.nearest[b] = near;
        }
    }
#endif
    __syncthreads();
    // ---- 5. 4x4 [R t; 0 1]
    if (tid < 16) {
        const int r = tid >> 2, c = tid & 3;
        float v;
        if (r == 3) {
            v = c == 3 ? 1.f : 0.f;
        } else if (c == 3) {
            float acc = 0.f;
            for (int k = 0; k < keep; ++k) acc += P[9 * sm.ord_tr[k] + 6 + r];
            v = acc / (float)keep;
        } else {  // quaternion_to_matrix (rotation_conversions.py:41-70)
            const float qr = sm.qavg[0], qi = sm.qavg[1], qj = sm.qavg[2], qk = sm.qavg[3];
            const float two_s = 2.0f / (((qr * qr + qi * qi) + qj * qj) + qk * qk);
            const float m[9] = {1 - two_s * (qj * qj + qk * qk), two_s * (qi * qj - qk * qr), two_s * (qi * qk + qj * qr),
                                two_s * (qi * qj + qk * qr), 1 - two_s * (qi * qi + qk * qk), two_s * (qj * qk - qi * qr),
                                two_s * (qi * qk - qj * qr), two_s * (qj * qk + qi * qr), 1 - two_s * (qi * qi + qj * qj)};
            v = 0.f;
#pragma unroll
            for (int e = 0; e < 9; ++e)
                if (e == r * 3 + c) v = m[e];
        }
        agg[(size_t)b * 16 + tid] = v;
#if AGG_MODES
        if (r < 3 && c < 3) ma.mode_pose[(size_t)b * ma.max_modes * 16 + tid] = v;
#endif
    }
