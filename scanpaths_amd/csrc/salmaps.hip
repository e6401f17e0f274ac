// Attention-map losses (AiR/models/loss.py:16-25, 47-170) and the saliency-map metrics AUC-Judd / NSS / KL-div
// (utils/evaltools/visual_attention_metrics.py:41-192).
//
// Losses (fp32 in and out, fp64 row arithmetic).  One launch computes the value AND the gradient coefficients; the host's backward
// scales the coefficients by grad_output (sp_scale_by for a scalar loss, sp_rowscale / sp_rowscale_idx for a per-row vector).
//   * map losses: one 256-thread workgroup per row of P elements.  The row is NOT held on chip: every pass re-reads it from global
//     memory (L2-resident at these sizes: <= 300 KB per row); passes per row -- NSS 3, CC 3, KLD 3, softmax-KLD 5.  Row sums are
//     per-thread strided fp64 accumulations, then wave64 shuffles and an LDS step in a fixed order (block_sum_d).
//   * the mean over rows: every workgroup writes its row value, takes a ticket (integer atomic), and the LAST one to arrive sums the
//     row values in row order and resets the ticket to 0 for the next launch -- no float atomics, so two calls are bit-identical.
//   * KLD_question_aligment: one workgroup per SAMPLE loops over its T step maps and its question objects (the min over steps and its
//     argmin stay in the workgroup, so the gradient goes to the chosen step in the same launch); 3 + (objects) passes per step map,
//     4 more per chosen step.
//   * DurationSmoothL1Loss / MLPRayleighDistribution / CC_MatchLoss: one workgroup over all elements (mask sum, then value+gradient).
// Metrics (fp64, one workgroup per map, one launch for a batch): see saliency_metrics_kernel; shuffled AUC, CC, SIM and information
// gain (Bylinskii et al. 2019; no counterpart in the reference): pool_counts_kernel and saliency_scores_kernel.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr double EPS = 1e-7;          // models/loss.py epsilon (a float in torch: promoted when it meets an fp32 tensor)

__device__ __forceinline__ double block_sum_d(double v, double* sh) {
    v = wave_sum_d(v);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
__device__ __forceinline__ double block_max_d(double v, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    return fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
}
__device__ __forceinline__ double block_min_d(double v, double* sh) { return -block_max_d(-v, sh); }
__device__ __forceinline__ int block_min_i(int v, int* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    return min(min(sh[0], sh[1]), min(sh[2], sh[3]));
}
__device__ __forceinline__ long long block_sum_ll(long long v, long long* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}

// true in every thread of the workgroup that arrives last among `n`; that workgroup then sees every other one's global writes.
// The ticket is back at 0 when the launch ends (the host hands in a zeroed word once and re-uses it on the same stream).
__device__ bool last_arrival(unsigned* ticket, unsigned n) {
    __shared__ int last;
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        const unsigned t = atomicAdd(ticket, 1u);
        last = (t == n - 1);
        if (last) atomicExch(ticket, 0u);
    }
    __syncthreads();
    if (last) __threadfence();
    return last;
}

// out[0] = scale * (sum of vals[0..n)), by the last workgroup: strided per-thread sums, then the fixed block tree (the same order on
// every call; a single thread walking the n values one load at a time cost ~80 us at n = 512)
__device__ void finish_sum(const float* vals, int n, double scale, unsigned* ticket, float* out) {
    __shared__ double shf[4];
    if (!last_arrival(ticket, (unsigned)gridDim.x)) return;
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += NT) s += (double)__builtin_nontemporal_load(vals + i);
    s = block_sum_d(s, shf);
    if (threadIdx.x == 0) out[0] = (float)(s * scale);
}
__device__ void finish_mean(const float* vals, int n, unsigned* ticket, float* out) { finish_sum(vals, n, 1.0 / (double)n, ticket, out); }

// ---------------------------------------------------------------------------------------------------------------------------
// NSS (loss.py:47-55): a = x / (max + eps); z = (a - mean) / (std_unbiased + eps); val = sum(z f) / (sum f + eps).
// d val / d a_j = (c_j - C/P) / D - N (a_j - mu) / (D^2 (P-1) s)     c = f / (Sf + eps), C = sum c, N = sum c (a - mu), D = s + eps
// d val / d x_j = g_a_j / (m + eps) - [j == argmax] sum_i g_a_i x_i / (m + eps)^2   (the max's gradient goes to its first index)
__global__ __launch_bounds__(NT) void nss_loss_kernel(const float* __restrict__ x, const float* __restrict__ f, int P, float scale,
                                                      float* __restrict__ row_val, float* __restrict__ coef, unsigned* ticket,
                                                      float* out) {
    __shared__ double sh[4];
    __shared__ int shi[4];
    const int r = blockIdx.x;
    const float* xr = x + (int64_t)r * P;
    const float* fr = f + (int64_t)r * P;
    float* cr = coef + (int64_t)r * P;
    double mx = -INFINITY, sx = 0.0, sf = 0.0;
    for (int i = threadIdx.x; i < P; i += NT) {
        const double v = xr[i];
        mx = fmax(mx, v);
        sx += v;
        sf += fr[i];
    }
    mx = block_max_d(mx, sh);
    sx = block_sum_d(sx, sh);
    sf = block_sum_d(sf, sh);
    int am = P;
    for (int i = threadIdx.x; i < P; i += NT)
        if ((double)xr[i] == mx) { am = i; break; }
    am = block_min_i(am, shi);
    const double me = mx + EPS, fe = sf + EPS, mu = sx / me / P;
    double saa = 0.0, n = 0.0, scx = 0.0, sax = 0.0;
    for (int i = threadIdx.x; i < P; i += NT) {
        const double v = xr[i], a = v / me - mu, c = fr[i] / fe;
        saa += a * a;
        n += c * a;
        scx += c * v;
        sax += a * v;
    }
    saa = block_sum_d(saa, sh);
    n = block_sum_d(n, sh);
    scx = block_sum_d(scx, sh);
    sax = block_sum_d(sax, sh);
    const double s = sqrt(saa / (P - 1)), D = s + EPS, C = sf / fe;
    const double k2 = n / (D * D * (P - 1) * s);
    const double gax = (scx - C / P * sx) / D - k2 * sax;
    for (int i = threadIdx.x; i < P; i += NT) {
        const double v = xr[i], a = v / me - mu;
        double g = ((fr[i] / fe - C / P) / D - k2 * a) / me;
        if (i == am) g -= gax / (me * me);
        cr[i] = (float)(g * scale);
    }
    if (threadIdx.x == 0) row_val[r] = (float)(n / D);
    finish_mean(row_val, gridDim.x, ticket, out);
}

// ---------------------------------------------------------------------------------------------------------------------------
// CC (loss.py:57-74): xn = x / (Sx + eps), centred xc; r = sum(xc yc) / (|xc| |yc| + eps).
// g_j = yc_j / D - K xc_j (K = cov |yc| / (D^2 |xc|)), h = g - mean(g) (the centring), d r / d x_j = h_j / (Sx+eps) - sum(h x) / (Sx+eps)^2
struct CCRow {
    double r, sx, D, K, mg, shx, mux, muy, xe, ye;
};
__device__ CCRow cc_row(const float* xr, const float* yr, int P, double* sh) {
    CCRow o;
    double sx = 0.0, sy = 0.0;
    for (int i = threadIdx.x; i < P; i += NT) {
        sx += xr[i];
        sy += yr[i];
    }
    sx = block_sum_d(sx, sh);
    sy = block_sum_d(sy, sh);
    o.xe = sx + EPS;
    o.ye = sy + EPS;
    o.mux = sx / o.xe / P;
    o.muy = sy / o.ye / P;
    double sxy = 0.0, sxx = 0.0, syy = 0.0, sxc = 0.0, syc = 0.0, syx = 0.0, sxcx = 0.0;
    for (int i = threadIdx.x; i < P; i += NT) {
        const double xv = xr[i], xc = xv / o.xe - o.mux, yc = yr[i] / o.ye - o.muy;
        sxy += xc * yc;
        sxx += xc * xc;
        syy += yc * yc;
        sxc += xc;
        syc += yc;
        syx += yc * xv;
        sxcx += xc * xv;
    }
    sxy = block_sum_d(sxy, sh);
    sxx = block_sum_d(sxx, sh);
    syy = block_sum_d(syy, sh);
    sxc = block_sum_d(sxc, sh);
    syc = block_sum_d(syc, sh);
    syx = block_sum_d(syx, sh);
    sxcx = block_sum_d(sxcx, sh);
    const double sgx = sqrt(sxx), sgy = sqrt(syy);
    o.sx = sx;
    o.D = sgx * sgy + EPS;
    o.r = sxy / o.D;
    o.K = sxy * sgy / (o.D * o.D * sgx);
    o.mg = (syc / o.D - o.K * sxc) / P;
    o.shx = syx / o.D - o.K * sxcx - o.mg * sx;
    return o;
}
__device__ void cc_grad(const float* xr, const float* yr, int P, const CCRow& o, double scale, float* cr) {
    for (int i = threadIdx.x; i < P; i += NT) {
        const double xc = xr[i] / o.xe - o.mux, yc = yr[i] / o.ye - o.muy;
        const double h = yc / o.D - o.K * xc - o.mg;
        cr[i] = (float)((h / o.xe - o.shx / (o.xe * o.xe)) * scale);
    }
}

__global__ __launch_bounds__(NT) void cc_loss_kernel(const float* __restrict__ x, const float* __restrict__ y, int P, float scale,
                                                     float* __restrict__ row_val, float* __restrict__ coef, unsigned* ticket,
                                                     float* out) {
    __shared__ double sh[4];
    const int r = blockIdx.x;
    const CCRow o = cc_row(x + (int64_t)r * P, y + (int64_t)r * P, P, sh);
    cc_grad(x + (int64_t)r * P, y + (int64_t)r * P, P, o, scale, coef + (int64_t)r * P);
    if (threadIdx.x == 0) row_val[r] = (float)o.r;
    finish_mean(row_val, gridDim.x, ticket, out);
}

// CC_terms (loss.py:76-98): rows with sum(good[b]) > 0 and sum(poor[b]) > 0 only, compacted in row order.  Every workgroup counts the
// paired rows itself (B*T mask reads), so the position of its row and the total need no second launch.
__device__ bool cc_paired(const float* good, const float* poor, int b, int T) {
    float g = 0.f, p = 0.f;
    for (int t = 0; t < T; ++t) {
        g += good[(int64_t)b * T + t];
        p += poor[(int64_t)b * T + t];
    }
    return g > 0.f && p > 0.f;
}
__global__ __launch_bounds__(NT) void cc_terms_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                      const float* __restrict__ good, const float* __restrict__ poor, int P, int T,
                                                      float* __restrict__ out, int* __restrict__ idx, int* __restrict__ count,
                                                      float* __restrict__ coef) {
    __shared__ double sh[4];
    __shared__ long long shl[4];
    const int r = blockIdx.x, R = gridDim.x;
    long long before = 0, total = 0;
    for (int b = threadIdx.x; b < R; b += NT) {
        const int pb = cc_paired(good, poor, b, T) ? 1 : 0;
        total += pb;
        before += (b < r) ? pb : 0;
    }
    before = block_sum_ll(before, shl);
    total = block_sum_ll(total, shl);
    const bool paired = cc_paired(good, poor, r, T);
    float* cr = coef + (int64_t)r * P;
    if (r == 0 && threadIdx.x == 0) count[0] = (int)total;
    if (!paired) {
        for (int i = threadIdx.x; i < P; i += NT) cr[i] = 0.f;
        if (threadIdx.x == 0) idx[r] = -1;
        return;
    }
    const CCRow o = cc_row(x + (int64_t)r * P, y + (int64_t)r * P, P, sh);
    cc_grad(x + (int64_t)r * P, y + (int64_t)r * P, P, o, 1.0, cr);
    if (threadIdx.x == 0) {
        idx[r] = (int)before;
        out[before] = (float)o.r;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// KLD (loss.py:104-126): p = x / (Sx + eps), q = y / (Sy + eps), val = sum q log(q / (p + eps) + eps).
// h_i = d val / d p_i = -q^2 / ((p + eps)^2 (q / (p + eps) + eps));  d val / d x_j = h_j / (Sx+eps) - sum(h x) / (Sx+eps)^2.
// SOFTMAX: x = softmax(z) over the row (two more passes: max, normaliser), d / d z_j = x_j (g_j - sum_i x_i g_i) with
// sum_i x_i g_i = sum(h x) eps / (Sx+eps)^2.  Y(i) supplies the target's element i.
struct KldRow {
    double zmax, zinv, xe;            // softmax max / 1 / normaliser (SOFTMAX), Sx + eps
};
template <bool SOFTMAX>
__device__ __forceinline__ double kld_x(const float* zr, int i, const KldRow& k) {
    return SOFTMAX ? exp((double)zr[i] - k.zmax) * k.zinv : (double)zr[i];
}
template <bool SOFTMAX>
__device__ KldRow kld_stats(const float* zr, int P, double* sh) {           // 1 pass (3 with the softmax)
    KldRow k{0.0, 1.0, 0.0};
    if (SOFTMAX) {
        double m = -INFINITY;
        for (int i = threadIdx.x; i < P; i += NT) m = fmax(m, (double)zr[i]);
        k.zmax = block_max_d(m, sh);
        double z = 0.0;
        for (int i = threadIdx.x; i < P; i += NT) z += exp((double)zr[i] - k.zmax);
        k.zinv = 1.0 / block_sum_d(z, sh);
    }
    double sx = 0.0;
    for (int i = threadIdx.x; i < P; i += NT) sx += kld_x<SOFTMAX>(zr, i, k);
    k.xe = block_sum_d(sx, sh) + EPS;
    return k;
}
// h_i x_i and the value term of element i
__device__ __forceinline__ void kld_elem(double xv, double q, double xe, double& val, double& hx) {
    const double p = xv / xe + EPS, u = q / p + EPS;
    val = q * log(u);
    hx = -q * q / (p * p * u) * xv;
}
// d val / d z_i (d / d x_i without the softmax), before any scale
template <bool SOFTMAX>
__device__ __forceinline__ double kld_grad_elem(double xv, double q, double xe, double shx) {
    const double p = xv / xe + EPS, u = q / p + EPS;
    const double g = -q * q / (p * p * u) / xe - shx / (xe * xe);
    return SOFTMAX ? xv * (g - shx * EPS / (xe * xe)) : g;
}
// one pass: (value, sum h x) against the target yat (sum of the target sy)
template <bool SOFTMAX, typename Y>
__device__ void kld_terms(const float* zr, int P, const KldRow& k, Y yat, double sy, double& val, double& shx, double* sh) {
    const double ye = sy + EPS;
    double v = 0.0, h = 0.0;
    for (int i = threadIdx.x; i < P; i += NT) {
        double a, c;
        kld_elem(kld_x<SOFTMAX>(zr, i, k), yat(i) / ye, k.xe, a, c);
        v += a;
        h += c;
    }
    val = block_sum_d(v, sh);
    shx = block_sum_d(h, sh);
}
template <bool SOFTMAX, typename Y>
__device__ double kld_row(const float* zr, int P, Y yat, double sy, double scale, float* cr, double* sh) {
    const KldRow k = kld_stats<SOFTMAX>(zr, P, sh);
    double val, shx;
    kld_terms<SOFTMAX>(zr, P, k, yat, sy, val, shx, sh);
    const double ye = sy + EPS;
    for (int i = threadIdx.x; i < P; i += NT)
        cr[i] = (float)(kld_grad_elem<SOFTMAX>(kld_x<SOFTMAX>(zr, i, k), yat(i) / ye, k.xe, shx) * scale);
    return val;
}

template <typename Y>
__device__ double row_sum(int P, Y yat, double* sh) {
    double s = 0.0;
    for (int i = threadIdx.x; i < P; i += NT) s += yat(i);
    return block_sum_d(s, sh);
}

// out == nullptr: KLD_items (row values are the result, coefficients unscaled)
__global__ __launch_bounds__(NT) void kld_loss_kernel(const float* __restrict__ x, const float* __restrict__ y, int P, float scale,
                                                      float* __restrict__ row_val, float* __restrict__ coef, unsigned* ticket,
                                                      float* out) {
    __shared__ double sh[4];
    const int r = blockIdx.x;
    const float* yr = y + (int64_t)r * P;
    auto yat = [&](int i) { return (double)yr[i]; };
    const double sy = row_sum(P, yat, sh);
    const double v = kld_row<false>(x + (int64_t)r * P, P, yat, sy, scale, coef + (int64_t)r * P, sh);
    if (threadIdx.x == 0) row_val[r] = (float)v;
    if (out) finish_mean(row_val, gridDim.x, ticket, out);
}

// KLD_visual_linguistic_alignment (loss.py:128-140): target = (sum_m qpos*qm + sum_m apos*am > 0) / count (no eps: 0/0 = NaN when a
// sample has no box), boxes channel-last [B][P][M]; prediction softmax(z) over the P pixels of the sample's single map.
__device__ __forceinline__ bool box_union(const float* qpos, const float* qm, int Mq, const float* apos, const float* am, int Ma,
                                          int b, int P, int i) {
    float s = 0.f, t = 0.f;
    const float* qp = qpos + ((int64_t)b * P + i) * Mq;
    for (int m = 0; m < Mq; ++m) s += qp[m] * qm[(int64_t)b * Mq + m];
    const float* ap = apos + ((int64_t)b * P + i) * Ma;
    for (int m = 0; m < Ma; ++m) t += ap[m] * am[(int64_t)b * Ma + m];
    return s + t > 0.f;
}
__global__ __launch_bounds__(NT) void kld_box_kernel(const float* __restrict__ z, const float* __restrict__ qpos,
                                                     const float* __restrict__ qm, int Mq, const float* __restrict__ apos,
                                                     const float* __restrict__ am, int Ma, int P, float scale,
                                                     float* __restrict__ row_val, float* __restrict__ coef, unsigned* ticket,
                                                     float* out) {
    __shared__ double sh[4];
    const int b = blockIdx.x;
    auto bin = [&](int i) { return box_union(qpos, qm, Mq, apos, am, Ma, b, P, i) ? 1.0 : 0.0; };
    const double cnt = row_sum(P, bin, sh);
    auto yat = [&](int i) { return (double)(float)(bin(i) / cnt); };
    const double sy = row_sum(P, yat, sh);
    const double v = kld_row<true>(z + (int64_t)b * P, P, yat, sy, scale, coef + (int64_t)b * P, sh);
    if (threadIdx.x == 0) row_val[b] = (float)v;
    finish_mean(row_val, gridDim.x, ticket, out);
}

// KLD_question_aligment (loss.py:142-170): one workgroup per sample b.  Objects m < (first zero of qmask[b]) pair with b; for each,
// kl[t] = KLD_items(softmax(z[b,t]), qpos[b,:,m]) with +inf where dmask[b,t] == 0, the pair's value is min_t kl[t] (first index on a
// tie), and its gradient (1 / total pairs) goes to that step only.  Every workgroup counts the total pairs itself (B*M mask reads).
constexpr int QA_MAX = 1024;            // T * M per sample held in LDS
__global__ __launch_bounds__(NT) void kld_question_kernel(const float* __restrict__ z, const float* __restrict__ qpos,
                                                          const float* __restrict__ qm, const float* __restrict__ dm, int T, int M,
                                                          int P, float* __restrict__ sample_sum, int* __restrict__ npairs,
                                                          float* __restrict__ coef, unsigned* ticket, float* out) {
    __shared__ double sh[4];
    __shared__ long long shl[4];
    __shared__ double kl[QA_MAX];
    __shared__ double shx[QA_MAX];
    __shared__ double sy[64];
    __shared__ int tstar[64];
    const int b = blockIdx.x, B = gridDim.x;
    long long tot = 0;
    for (int s = threadIdx.x; s < B; s += NT) {
        int k = 0;
        while (k < M && qm[(int64_t)s * M + k] != 0.f) ++k;
        tot += k;
    }
    tot = block_sum_ll(tot, shl);
    int nb = 0;
    while (nb < M && qm[(int64_t)b * M + nb] != 0.f) ++nb;
    const double inv_pairs = 1.0 / (double)tot;
    for (int m = 0; m < nb; ++m) {
        const double s = row_sum(P, [&](int i) { return (double)qpos[((int64_t)b * P + i) * M + m]; }, sh);
        if (threadIdx.x == 0) sy[m] = s;
    }
    __syncthreads();
    // values: the softmax statistics once per step, then one pass per object
    for (int t = 0; t < T; ++t) {
        const float* zr = z + ((int64_t)b * T + t) * P;
        if (dm[(int64_t)b * T + t] == 0.f) {
            if (threadIdx.x == 0)
                for (int m = 0; m < nb; ++m) kl[t * M + m] = INFINITY;
            continue;
        }
        const KldRow k = kld_stats<true>(zr, P, sh);
        for (int m = 0; m < nb; ++m) {
            double v, h;
            kld_terms<true>(zr, P, k, [&](int i) { return (double)qpos[((int64_t)b * P + i) * M + m]; }, sy[m], v, h, sh);
            if (threadIdx.x == 0) {
                kl[t * M + m] = v;
                shx[t * M + m] = h;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int m = 0; m < nb; ++m) {
            int best = 0;
            for (int t = 1; t < T; ++t)
                if (kl[t * M + m] < kl[best * M + m]) best = t;
            s += kl[best * M + m];
            tstar[m] = kl[best * M + m] < INFINITY ? best : -1;
        }
        sample_sum[b] = (float)s;
        if (b == 0) npairs[0] = (int)tot;
    }
    __syncthreads();
    // gradients: the rows of the chosen steps (summed over the objects whose min a step holds), exact zeros elsewhere
    for (int t = 0; t < T; ++t) {
        float* cr = coef + ((int64_t)b * T + t) * P;
        bool chosen = false;
        for (int m = 0; m < nb; ++m) chosen |= tstar[m] == t;
        if (!chosen) {
            for (int i = threadIdx.x; i < P; i += NT) cr[i] = 0.f;
            continue;
        }
        const float* zr = z + ((int64_t)b * T + t) * P;
        const KldRow k = kld_stats<true>(zr, P, sh);
        for (int i = threadIdx.x; i < P; i += NT) {
            const double xv = kld_x<true>(zr, i, k);
            double g = 0.0;
            for (int m = 0; m < nb; ++m)
                if (tstar[m] == t)
                    g += kld_grad_elem<true>(xv, qpos[((int64_t)b * P + i) * M + m] / (sy[m] + EPS), k.xe, shx[t * M + m]);
            cr[i] = (float)(g * inv_pairs);
        }
    }
    finish_sum(sample_sum, B, inv_pairs, ticket, out);
}

// ---------------------------------------------------------------------------------------------------------------------------
// DurationSmoothL1Loss (loss.py:16-19) and MLPRayleighDistribution (loss.py:21-25): one workgroup over all n elements.
template <int KIND>
__global__ __launch_bounds__(NT) void masked_elem_kernel(const float* __restrict__ x, const float* __restrict__ gt,
                                                         const float* __restrict__ mask, int64_t n, float* __restrict__ out,
                                                         float* __restrict__ coef) {
    __shared__ double sh[4];
    double ms = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += NT) ms += mask[i];
    ms = block_sum_d(ms, sh);
    const double inv = 1.0 / ms;
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += NT) {
        const float m = mask[i];
        double g = 0.0;
        if (KIND == 0) {            // smooth L1, beta = 1, sum; gradient of input*mask
            const double d = (double)(x[i] * m) - (double)(gt[i] * m), a = fabs(d);
            acc += a < 1.0 ? 0.5 * d * d : a - 0.5;
            g = (a < 1.0 ? d : (d > 0.0 ? 1.0 : -1.0)) * (double)m;
        } else if (m == 1.f) {      // Rayleigh: -[log(gt/s2 + eps) - gt^2/(2 s2)], gradient w.r.t. s2
            const double s2 = x[i], d = gt[i], u = d / s2 + EPS;
            acc -= log(u) - d * d / (2.0 * s2);
            g = (d / (s2 * s2)) / u - d * d / (2.0 * s2 * s2);
        }
        coef[i] = (float)(g * inv);
    }
    acc = block_sum_d(acc, sh);
    if (threadIdx.x == 0) out[0] = (float)(acc * inv);
}

// CC_MatchLoss (loss.py:100-102): mean |a - b|, coefficients sign(a - b) / n and -sign(a - b) / n (sign(0) = 0, as torch's abs backward)
__global__ __launch_bounds__(NT) void abs_diff_mean_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t n,
                                                           float* __restrict__ out, float* __restrict__ ca, float* __restrict__ cb) {
    __shared__ double sh[4];
    double acc = 0.0;
    const float inv = (float)(1.0 / (double)n);
    for (int64_t i = threadIdx.x; i < n; i += NT) {
        const float d = a[i] - b[i];
        acc += fabsf(d);
        const float s = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
        ca[i] = s * inv;
        cb[i] = -s * inv;
    }
    acc = block_sum_d(acc, sh);
    if (threadIdx.x == 0) out[0] = (float)(acc / (double)n);
}

// out[r, i] = coef[r, i] * g[idx[r]] (0 where idx[r] < 0): the backward of a loss that returns a compacted subset of its rows
__global__ __launch_bounds__(NT) void rowscale_idx_kernel(const float* coef, const float* g, const int* idx, int64_t n, int P,
                                                          float* out) {
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        const int k = idx[i / P];
        out[i] = k < 0 ? 0.f : coef[i] * g[k];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Saliency-map metrics, float64, one 256-thread workgroup per map (visual_attention_metrics.py:41-192):
//   AUC-Judd: S + jitter, min-max normalised; the fixated values (F > 0) sorted in descending order are the thresholds t_k.
//     Every pixel finds by binary search the first k with t_k <= S_i and adds 1 to hist[k]; the inclusive prefix sum of hist is
//     then exactly #(S >= t_k) for every k at once (O(P log Nfix)), and the ROC points and np.trapz follow.  Thresholds and the
//     histogram sit in LDS up to SM_LDS_FIX fixations (bitonic sort in LDS), else in the map's slice of a global scratch buffer the
//     host sizes from the fixation counts (same code on a global pointer).
//   NSS: S / max (max != 0), standardised with std(ddof=1) (!= 0), mean at F != 0.   KLdiv: eps 1e-12 with the any() guards.
// All sums are per-thread strided, then a fixed-order block tree: within ~1e-15 relative of numpy's pairwise sums.
constexpr int SM_LDS_FIX = 2048;

__device__ void bitonic_desc(double* a, int n2) {
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n2; i += NT) {
                const int l = i ^ j;
                if (l > i) {
                    const double ai = a[i], al = a[l];
                    const bool desc = (i & k) == 0;
                    if (desc ? (ai < al) : (ai > al)) {
                        a[i] = al;
                        a[l] = ai;
                    }
                }
            }
            __syncthreads();
        }
}

// in place: h[k] <- h[0] + ... + h[k], n entries
__device__ void block_inclusive_scan(int* h, int n, long long* part) {
    const int chunk = (n + NT - 1) / NT, lo = min(n, (int)threadIdx.x * chunk), hi = min(n, lo + chunk);
    long long s = 0;
    for (int i = lo; i < hi; ++i) s += h[i];
    __syncthreads();
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long run = 0;
        for (int i = 0; i < NT; ++i) {
            const long long v = part[i];
            part[i] = run;
            run += v;
        }
    }
    __syncthreads();
    long long run = part[threadIdx.x];
    for (int i = lo; i < hi; ++i) {
        run += h[i];
        h[i] = (int)run;
    }
    __syncthreads();
}

__global__ __launch_bounds__(NT) void saliency_metrics_kernel(const double* __restrict__ sal, const double* __restrict__ fix,
                                                              const double* __restrict__ jitter, int P,
                                                              const int64_t* __restrict__ scratch_off, char* scratch,
                                                              double* __restrict__ auc, double* __restrict__ nss,
                                                              double* __restrict__ kld) {
    __shared__ double sh[4];
    __shared__ long long shl[4];
    __shared__ long long part[NT];
    __shared__ double thr_lds[SM_LDS_FIX];
    __shared__ int hist_lds[SM_LDS_FIX];
    __shared__ int fill;
    const int n = blockIdx.x;
    const double* S = sal + (int64_t)n * P;
    const double* F = fix + (int64_t)n * P;
    const double* J = jitter ? jitter + (int64_t)n * P : nullptr;
    auto sj = [&](int i) { return J ? S[i] + J[i] : S[i]; };
    // pass 1
    double vmin = INFINITY, vmax = -INFINITY, smax = -INFINITY, ssum = 0.0, fsum = 0.0;
    long long nfix = 0, nnz = 0, snz = 0;
    for (int i = threadIdx.x; i < P; i += NT) {
        const double v = sj(i), s = S[i], f = F[i];
        vmin = fmin(vmin, v);
        vmax = fmax(vmax, v);
        smax = fmax(smax, s);
        ssum += s;
        fsum += f;
        nfix += f > 0.0;
        nnz += f != 0.0;
        snz += s != 0.0;
    }
    vmin = block_min_d(vmin, sh);
    vmax = block_max_d(vmax, sh);
    smax = block_max_d(smax, sh);
    ssum = block_sum_d(ssum, sh);
    fsum = block_sum_d(fsum, sh);
    nfix = block_sum_ll(nfix, shl);
    nnz = block_sum_ll(nnz, shl);
    snz = block_sum_ll(snz, shl);

    // ---- KLdiv ----
    {
        double acc = 0.0;
        for (int i = threadIdx.x; i < P; i += NT) {
            const double m1 = snz ? S[i] / ssum : S[i], m2 = nnz ? F[i] / fsum : F[i];
            acc += m2 * log(1e-12 + m2 / (m1 + 1e-12));
        }
        acc = block_sum_d(acc, sh);
        if (threadIdx.x == 0) kld[n] = acc;
    }
    // ---- NSS ----
    {
        auto m1 = [&](int i) { return smax != 0.0 ? S[i] / smax : S[i]; };
        double s = 0.0;
        for (int i = threadIdx.x; i < P; i += NT) s += m1(i);
        const double mean = block_sum_d(s, sh) / P;
        double q = 0.0;
        for (int i = threadIdx.x; i < P; i += NT) {
            const double d = m1(i) - mean;
            q += d * d;
        }
        const double sd = sqrt(block_sum_d(q, sh) / (P - 1));
        double a = 0.0;
        for (int i = threadIdx.x; i < P; i += NT)
            if (F[i] != 0.0) a += sd != 0.0 ? (m1(i) - mean) / sd : m1(i);
        a = block_sum_d(a, sh);
        if (threadIdx.x == 0) nss[n] = nnz ? a / (double)nnz : NAN;
    }
    // ---- AUC-Judd ----
    const double range = vmax - vmin;
    auto norm = [&](int i) { return (sj(i) - vmin) / range; };
    long long finite = 0;
    for (int i = threadIdx.x; i < P; i += NT) finite += !isnan(norm(i));
    finite = block_sum_ll(finite, shl);
    if (nnz == 0 || finite == 0) {
        if (threadIdx.x == 0) auc[n] = NAN;
        return;
    }
    const int nf = (int)nfix;
    int n2 = 1;
    while (n2 < nf) n2 <<= 1;
    double* thr = thr_lds;
    int* hist = hist_lds;
    if (nf > SM_LDS_FIX) {
        const int64_t need = (int64_t)n2 * 8 + (int64_t)nf * 4;
        if (!scratch || scratch_off[n] < 0 || scratch_off[n + 1] - scratch_off[n] < need) {     // host sized it otherwise: refuse
            if (threadIdx.x == 0) auc[n] = NAN;
            return;
        }
        thr = (double*)(scratch + scratch_off[n]);
        hist = (int*)(scratch + scratch_off[n] + (int64_t)n2 * 8);
    }
    if (threadIdx.x == 0) fill = 0;
    for (int i = threadIdx.x; i < n2; i += NT) thr[i] = -INFINITY;
    for (int i = threadIdx.x; i < nf; i += NT) hist[i] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < P; i += NT)
        if (F[i] > 0.0) {
            const int k = atomicAdd(&fill, 1);
            if (k < nf) thr[k] = norm(i);
        }
    __syncthreads();
    if (nf > 1) bitonic_desc(thr, n2);
    for (int i = threadIdx.x; i < P; i += NT) {
        const double v = norm(i);
        int lo = 0, hi = nf;                  // first k with thr[k] <= v (thr descending)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (thr[mid] <= v) hi = mid;
            else lo = mid + 1;
        }
        if (lo < nf) atomicAdd(&hist[lo], 1);
    }
    __syncthreads();
    if (nf > 0) block_inclusive_scan(hist, nf, part);
    // np.trapz(tp, x=fp) over the nf + 2 ROC points: term j (1..nf+1) = (fp[j] - fp[j-1]) * (tp[j] + tp[j-1]) / 2
    const double negs = (double)(P - nf);
    auto fp = [&](int j) { return j == 0 ? 0.0 : j > nf ? 1.0 : (double)(hist[j - 1] - (j - 1)) / negs; };
    auto tp = [&](int j) { return j == 0 ? 0.0 : j > nf ? 1.0 : (double)j / (double)nf; };
    const int nt = nf + 1, chunk = (nt + NT - 1) / NT, lo = min(nt, (int)threadIdx.x * chunk), hi = min(nt, lo + chunk);
    double acc = 0.0;
    for (int j = lo + 1; j <= hi; ++j) acc += (fp(j) - fp(j - 1)) * (tp(j) + tp(j - 1)) / 2.0;
    acc = block_sum_d(acc, sh);
    if (threadIdx.x == 0) auc[n] = acc;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The pool of shuffled-AUC negatives: cnt[e][p] = #(maps g of image e with F_g[p] > 0), tot[p] = sum_e cnt[e][p].  One thread owns
// pixel p for every map and image (its loads are coalesced across the wave), so the counts need neither atomics nor a zeroed buffer.
// Maps are read eight at a time so that the loads are in flight together and not behind the count updates.
__global__ __launch_bounds__(NT) void pool_counts_kernel(const double* __restrict__ fix, const int* __restrict__ cls, int G, int P, int E,
                                                         int* __restrict__ cnt, int* __restrict__ tot) {
    const int p = blockIdx.x * NT + threadIdx.x;
    if (p >= P) return;
    for (int e = 0; e < E; ++e) cnt[(int64_t)e * P + p] = 0;
    int t = 0;
    for (int g0 = 0; g0 < G; g0 += 8) {
        double f[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) f[k] = g0 + k < G ? fix[(int64_t)(g0 + k) * P + p] : 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (f[k] > 0.0) {
                const int c = cls[g0 + k];
                if (c >= 0 && c < E) {            // the host checked; a stray value must not write outside cnt
                    cnt[(int64_t)c * P + p] += 1;
                    ++t;
                }
            }
    }
    tot[p] = t;
}

// Shuffled AUC, CC, SIM and information gain, float64, one 256-thread workgroup per map (include/scanpaths_amd.h sp_saliency_scores).
//   pass 1: the sums of S, D, Bm, the fixated-pixel count n, the pool weight W (int64) and the NaN count of S;
//   pass 2: the centred products of CC, the min terms of SIM and, at fixated pixels, the log2 terms of IG;
//   sAUC:   the fixated values sorted in descending order (bitonic, in LDS up to SM_LDS_FIX, else in the map's scratch slice).  A pool
//     pixel of value v and weight w then finds by two binary searches how many fixated values lie above v (a) and at or above v (b)
//     and adds w * (a + b) to its thread's int64: summed over the pool this is sum_i (2 below_i + equal_i) -- the histogram and prefix
//     sum of AUC-Judd collapse, since sum_i prefix[i] = sum_k hist[k] (n - k).  Integer sums: the result does not depend on order.
// Double sums: per-thread strided, then the fixed block tree (as above).
constexpr double IG_EPS = 2.220446049250313e-16;
__global__ __launch_bounds__(NT) void saliency_scores_kernel(const double* __restrict__ sal, const double* __restrict__ fix,
                                                             const double* __restrict__ dens, const double* __restrict__ base,
                                                             const int* __restrict__ pool, int64_t pool_stride,
                                                             const int* __restrict__ cnt, const int* __restrict__ cls, int E, int P,
                                                             double alpha, const int64_t* __restrict__ scratch_off, char* scratch,
                                                             double* __restrict__ sauc, double* __restrict__ cc,
                                                             double* __restrict__ sim, double* __restrict__ ig) {
    __shared__ double sh[4];
    __shared__ long long shl[4];
    __shared__ double thr_lds[SM_LDS_FIX];
    __shared__ int fill;
    const int n = blockIdx.x;
    const double* S = sal + (int64_t)n * P;
    const double* F = fix ? fix + (int64_t)n * P : nullptr;
    const double* D = dens ? dens + (int64_t)n * P : nullptr;
    const double* B = base ? base + (int64_t)n * P : nullptr;
    const bool do_auc = sauc && F && pool, do_cc = cc && D, do_sim = sim && D, do_ig = ig && F && B;
    const int* T = pool ? pool + (int64_t)n * pool_stride : nullptr;
    const int* C = nullptr;
    bool cls_ok = true;
    if (cnt) {
        const int c = cls[n];
        cls_ok = c >= 0 && c < E;
        if (cls_ok) C = cnt + (int64_t)c * P;
    }
    auto wt = [&](int i) { return C ? T[i] - C[i] : T[i]; };
    // pass 1
    double sS = 0.0, sD = 0.0, sB = 0.0;
    long long nfix = 0, W = 0, nanS = 0;
    for (int i = threadIdx.x; i < P; i += NT) {
        const double s = S[i];
        sS += s;
        nanS += isnan(s);
        if (D) sD += D[i];
        if (B) sB += B[i];
        if (F) nfix += F[i] > 0.0;
        if (do_auc && cls_ok) {
            const int w = wt(i);
            W += w > 0 ? w : 0;
        }
    }
    sS = block_sum_d(sS, sh);
    sD = block_sum_d(sD, sh);
    sB = block_sum_d(sB, sh);
    nfix = block_sum_ll(nfix, shl);
    W = block_sum_ll(W, shl);
    nanS = block_sum_ll(nanS, shl);
    // pass 2: CC, SIM, IG
    if (do_cc || do_sim || do_ig) {
        const double mS = sS / P, mD = sD / P, ka = 1.0 - alpha, ua = alpha / P;
        double cxy = 0.0, cxx = 0.0, cyy = 0.0, smin = 0.0, gain = 0.0;
        for (int i = threadIdx.x; i < P; i += NT) {
            const double s = S[i];
            if (D) {
                const double d = D[i], a = s - mS, b = d - mD;
                cxy += a * b;
                cxx += a * a;
                cyy += b * b;
                smin += fmin(s / sS, d / sD);
            }
            if (do_ig && F[i] > 0.0) gain += log2(IG_EPS + (ka * s / sS + ua)) - log2(IG_EPS + (ka * B[i] / sB + ua));
        }
        cxy = block_sum_d(cxy, sh);
        cxx = block_sum_d(cxx, sh);
        cyy = block_sum_d(cyy, sh);
        smin = block_sum_d(smin, sh);
        gain = block_sum_d(gain, sh);
        if (threadIdx.x == 0) {
            const bool okS = sS > 0.0 && isfinite(sS), okD = sD > 0.0 && isfinite(sD), okB = sB > 0.0 && isfinite(sB);
            if (do_cc) cc[n] = (cxx > 0.0 && cyy > 0.0 && isfinite(cxx) && isfinite(cyy)) ? cxy / sqrt(cxx * cyy) : NAN;
            if (do_sim) sim[n] = (okS && okD) ? smin : NAN;
            if (do_ig) ig[n] = (nfix > 0 && okS && okB) ? gain / (double)nfix : NAN;
        }
    }
    if (!do_auc) return;
    // ---- sAUC ----
    const int nf = (int)nfix;
    int n2 = 1;
    while (n2 < nf) n2 <<= 1;
    double* thr = thr_lds;
    bool ok = cls_ok && nf > 0 && W > 0 && nanS == 0;
    if (ok && nf > SM_LDS_FIX) {
        if (!scratch || scratch_off[n] < 0 || scratch_off[n + 1] - scratch_off[n] < (int64_t)n2 * 8) ok = false;      // host sized it otherwise
        else thr = (double*)(scratch + scratch_off[n]);
    }
    if (!ok) {                                   // uniform over the workgroup: every term comes from a block sum
        if (threadIdx.x == 0) sauc[n] = NAN;
        return;
    }
    if (threadIdx.x == 0) fill = 0;
    for (int i = threadIdx.x; i < n2; i += NT) thr[i] = -INFINITY;
    __syncthreads();
    for (int i = threadIdx.x; i < P; i += NT)
        if (F[i] > 0.0) {
            const int k = atomicAdd(&fill, 1);
            if (k < nf) thr[k] = S[i];
        }
    __syncthreads();
    if (nf > 1) bitonic_desc(thr, n2);
    long long num = 0;
    for (int i = threadIdx.x; i < P; i += NT) {
        const int w = wt(i);
        if (w <= 0) continue;
        const double v = S[i];
        int lo = 0, hi = nf;                     // a = #(thr > v) = the first k with thr[k] <= v
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (thr[mid] <= v) hi = mid;
            else lo = mid + 1;
        }
        const int a = lo;
        hi = nf;                                 // b = #(thr >= v) = the first k >= a with thr[k] < v
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (thr[mid] < v) hi = mid;
            else lo = mid + 1;
        }
        num += (long long)w * (a + lo);
    }
    num = block_sum_ll(num, shl);
    if (threadIdx.x == 0) sauc[n] = (double)num / (double)(2LL * nf * W);
}

}  // namespace

extern "C" int sp_smooth_l1_loss(const float* x, const float* gt, const float* mask, int64_t n, float* out, float* coef, void* stream) {
    if (!x || !gt || !mask || !out || !coef) return SP_ENULL;
    if (n < 1) return SP_EINVAL;
    hipLaunchKernelGGL(masked_elem_kernel<0>, dim3(1), dim3(NT), 0, (hipStream_t)stream, x, gt, mask, n, out, coef);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_rayleigh_loss(const float* sigma2, const float* gt, const float* mask, int64_t n, float* out, float* coef,
                                void* stream) {
    if (!sigma2 || !gt || !mask || !out || !coef) return SP_ENULL;
    if (n < 1) return SP_EINVAL;
    hipLaunchKernelGGL(masked_elem_kernel<1>, dim3(1), dim3(NT), 0, (hipStream_t)stream, sigma2, gt, mask, n, out, coef);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_abs_diff_mean(const float* a, const float* b, int64_t n, float* out, float* coef_a, float* coef_b, void* stream) {
    if (!a || !b || !out || !coef_a || !coef_b) return SP_ENULL;
    if (n < 1) return SP_EINVAL;
    hipLaunchKernelGGL(abs_diff_mean_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, a, b, n, out, coef_a, coef_b);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_nss_loss(const float* x, const float* fix, int R, int P, float* out, float* row_val, float* coef, unsigned* ticket,
                           void* stream) {
    if (!x || !fix || !out || !row_val || !coef || !ticket) return SP_ENULL;
    if (R < 1 || P < 2) return SP_EINVAL;
    hipLaunchKernelGGL(nss_loss_kernel, dim3(R), dim3(NT), 0, (hipStream_t)stream, x, fix, P, 1.f / R, row_val, coef, ticket, out);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_cc_loss(const float* x, const float* y, int R, int P, float* out, float* row_val, float* coef, unsigned* ticket,
                          void* stream) {
    if (!x || !y || !out || !row_val || !coef || !ticket) return SP_ENULL;
    if (R < 1 || P < 1) return SP_EINVAL;
    hipLaunchKernelGGL(cc_loss_kernel, dim3(R), dim3(NT), 0, (hipStream_t)stream, x, y, P, 1.f / R, row_val, coef, ticket, out);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_cc_terms(const float* x, const float* y, const float* good, const float* poor, int R, int P, int T, float* out,
                           int* idx, int* count, float* coef, void* stream) {
    if (!x || !y || !good || !poor || !out || !idx || !count || !coef) return SP_ENULL;
    if (R < 1 || P < 1 || T < 1) return SP_EINVAL;
    hipLaunchKernelGGL(cc_terms_kernel, dim3(R), dim3(NT), 0, (hipStream_t)stream, x, y, good, poor, P, T, out, idx, count, coef);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_kld_loss(const float* x, const float* y, int R, int P, float* out, float* row_val, float* coef, unsigned* ticket,
                           void* stream) {
    if (!x || !y || !row_val || !coef || (out && !ticket)) return SP_ENULL;
    if (R < 1 || P < 1) return SP_EINVAL;
    hipLaunchKernelGGL(kld_loss_kernel, dim3(R), dim3(NT), 0, (hipStream_t)stream, x, y, P, out ? 1.f / R : 1.f, row_val, coef, ticket,
                       out);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_kld_box_alignment(const float* z, const float* qpos, const float* qmask, int Mq, const float* apos,
                                    const float* amask, int Ma, int B, int P, float* out, float* row_val, float* coef,
                                    unsigned* ticket, void* stream) {
    if (!z || !qpos || !qmask || !apos || !amask || !out || !row_val || !coef || !ticket) return SP_ENULL;
    if (B < 1 || P < 1 || Mq < 0 || Ma < 0) return SP_EINVAL;
    hipLaunchKernelGGL(kld_box_kernel, dim3(B), dim3(NT), 0, (hipStream_t)stream, z, qpos, qmask, Mq, apos, amask, Ma, P, 1.f / B,
                       row_val, coef, ticket, out);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_kld_question_alignment(const float* z, const float* qpos, const float* qmask, const float* dmask, int B, int T,
                                         int P, int M, float* out, int* npairs, float* sample_sum, float* coef, unsigned* ticket,
                                         void* stream) {
    if (!z || !qpos || !qmask || !dmask || !out || !npairs || !sample_sum || !coef || !ticket) return SP_ENULL;
    if (B < 1 || T < 1 || P < 1 || M < 1 || M > 64 || T * M > QA_MAX) return SP_EINVAL;
    hipLaunchKernelGGL(kld_question_kernel, dim3(B), dim3(NT), 0, (hipStream_t)stream, z, qpos, qmask, dmask, T, M, P, sample_sum,
                       npairs, coef, ticket, out);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_rowscale_idx(const float* coef, const float* g, const int* idx, int R, int P, float* out, void* stream) {
    if (!coef || !g || !idx || !out) return SP_ENULL;
    if (R < 1 || P < 1) return SP_EINVAL;
    const int64_t n = (int64_t)R * P;
    hipLaunchKernelGGL(rowscale_idx_kernel, dim3(sp_ew_grid(n, 2048, NT)), dim3(NT), 0, (hipStream_t)stream, coef, g, idx, n, P, out);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_saliency_metrics_lds_fixations(void) { return SM_LDS_FIX; }

extern "C" int sp_saliency_metrics(const double* sal, const double* fix, const double* jitter, int N, int P, const int64_t* scratch_off,
                                   void* scratch, double* auc, double* nss, double* kld, void* stream) {
    if (!sal || !fix || !scratch_off || !auc || !nss || !kld) return SP_ENULL;
    if (N < 1 || P < 1) return SP_EINVAL;
    hipLaunchKernelGGL(saliency_metrics_kernel, dim3(N), dim3(NT), 0, (hipStream_t)stream, sal, fix, jitter, P, scratch_off,
                       (char*)scratch, auc, nss, kld);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_fixation_pool_counts(const double* fix, const int* cls, int G, int P, int E, int* cls_dev, int* cnt, int* tot,
                                       void* stream) {
    if (!fix || !cls || !cls_dev || !cnt || !tot) return SP_ENULL;
    if (G < 1 || P < 1 || E < 1) return SP_EINVAL;
    for (int g = 0; g < G; ++g)
        if (cls[g] < 0 || cls[g] >= E) return SP_EINVAL;
    const hipError_t e = hipMemcpyAsync(cls_dev, cls, (size_t)G * sizeof(int), hipMemcpyHostToDevice, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pool_counts_kernel, dim3((unsigned)sp_cdiv(P, NT)), dim3(NT), 0, (hipStream_t)stream, fix, cls_dev, G, P, E, cnt,
                       tot);
    SP_LAUNCH_CHECK();
    return SP_OK;
}

extern "C" int sp_saliency_scores(const double* sal, const double* fix, const double* dens, const double* base, const int* pool,
                                  int64_t pool_stride, const int* cnt, const int* cls, int E, int N, int P, double uniform_mix,
                                  const int64_t* scratch_off, void* scratch, double* sauc, double* cc, double* sim, double* ig,
                                  void* stream) {
    const bool do_auc = sauc && fix && pool, do_ig = ig && fix && base;
    if (!sal || (!cnt != !cls) || !(do_auc || do_ig || (dens && (cc || sim))) || (do_auc && !scratch_off)) return SP_ENULL;
    if (N < 1 || P < 1) return SP_EINVAL;
    if (do_auc && ((pool_stride != 0 && pool_stride != P) || (cnt && E < 1))) return SP_EINVAL;
    if (do_ig && !(uniform_mix >= 0.0 && uniform_mix <= 1.0)) return SP_EINVAL;
    hipLaunchKernelGGL(saliency_scores_kernel, dim3(N), dim3(NT), 0, (hipStream_t)stream, sal, fix, dens, base, pool, pool_stride, cnt,
                       cls, E, P, uniform_mix, scratch_off, (char*)scratch, sauc, cc, sim, ig);
    SP_LAUNCH_CHECK();
    return SP_OK;
}
