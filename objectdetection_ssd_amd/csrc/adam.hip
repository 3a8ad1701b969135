// Fused Adam / AdamW step over the flat parameter store: torch.optim.Adam's update rule as one launch per flat range, driven by the
// same device words as the scheduled SGD launch (learning rate, EMA weight, clip scale, skip flag) plus a small state block of its own
// that holds the step counter and the running products beta1^t, beta2^t.  Nothing here depends on a host value that changes from step
// to step -- the bias corrections are formed on the device from the block -- so a captured train step replays for a whole run.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int ADAM_THREADS = 256;
constexpr int ADAM_MAX_BLOCKS = 2048;    // the grid rule of sgd_sched_kernel: 8 workgroups per CU on 256 CUs resident, the rest is grid-stride

inline int adam_blocks(size_t units) {
    const size_t b = (units + ADAM_THREADS - 1) / ADAM_THREADS;
    return (int)(b > (size_t)ADAM_MAX_BLOCKS ? ADAM_MAX_BLOCKS : (b ? b : 1));
}

// state: [0] pow1 (f64) | [1] pow2 (f64) | [2] low half: step (int32), high half spare.  One IEEE multiply per product and step.
__global__ __launch_bounds__(64) void adam_advance_kernel(double* __restrict__ state, double beta1, double beta2, const int* __restrict__ skip) {
    if (skip && *skip != 0) return;
    if (threadIdx.x != 0) return;
    int* step = reinterpret_cast<int*>(state + 2);
    state[0] = state[0] * beta1;
    state[1] = state[1] * beta2;
    step[0] = step[0] + 1;
}

// What one launch holds per thread besides the data: every value is rounded to f32 once, on the host or at the head of the kernel.
struct AdamScalars {
    float omb1, omb2, b2;      // f32(1 - beta1), f32(1 - beta2), f32(beta2)
    float eps, wd;
    float neg_step, bc2_sqrt;  // f32(-lr / (1 - pow1)), f32(sqrt(1 - pow2))
    float decay;               // decoupled form: f32(1 - lr * wd)
    float sc, ema_w;
    bool scaled, decoupled, has_wd;   // has_wd: the weight decay as given (f64) is not zero
};

// torch.optim.Adam's single-tensor sequence (lerp_, mul_ + addcmul_, sqrt / div / add_, addcdiv_); every fma is explicit.  Then, with
// EMA, the three separately rounded operations of sgd_element<true> on the parameter just formed.
template <bool EMA>
__device__ __forceinline__ void adam_element(float& p, const float g, float& m, float& v, float& e, const AdamScalars& s) {
    float gs = s.scaled ? g * s.sc : g;
    float w = p;
    if (s.has_wd) {
        if (s.decoupled) w = w * s.decay;
        else gs = __builtin_fmaf(s.wd, w, gs);
    }
    const float dm = gs - m;
    m = __builtin_fmaf(s.omb1, dm, m);
    const float g2 = s.omb2 * gs;
    const float vb = v * s.b2;
    v = __builtin_fmaf(g2, gs, vb);
    const float q = __builtin_sqrtf(v) / s.bc2_sqrt;
    const float den = q + s.eps;
    const float num = s.neg_step * m;
    const float upd = num / den;
    w = w + upd;
    p = w;
    if (EMA) {
        const float diff = w - e;
        const float mm = s.ema_w * diff;
        e = e + mm;
    }
}

// VEC: the ranges are 16-byte aligned and a multiple of 4 floats long, `n` counts 16-byte units.  Nine dword streams per element with
// EMA (p, g, m, v, e in; p, m, v, e out), seven without.  Gradient, both moments and the EMA are touched once per step and by nothing
// else before the next one: their vector accesses are non-temporal, the parameters' are plain (sgd_sched_kernel, for its reason).
template <bool VEC, bool EMA>
__global__ __launch_bounds__(ADAM_THREADS) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                            float* __restrict__ v, float* __restrict__ ema, size_t n, double lr,
                                                            const float* __restrict__ lr_dev, const float* __restrict__ ema_w_dev,
                                                            const double* __restrict__ state, AdamScalars s, double wd64,
                                                            const float* __restrict__ scale, const int* __restrict__ skip) {
    if (skip && *skip != 0) return;
    // one f64 division and one f64 square root per thread, none per element
    const double rate = lr_dev ? (double)*lr_dev : lr;
    const double pow1 = state[0], pow2 = state[1];
    s.neg_step = (float)(-(rate / (1.0 - pow1)));
    s.bc2_sqrt = (float)__builtin_sqrt(1.0 - pow2);
    s.decay = (float)(1.0 - rate * wd64);
    s.sc = scale ? *scale : 1.f;
    s.scaled = scale != nullptr;
    s.ema_w = EMA ? *ema_w_dev : 0.f;
    const size_t stride = (size_t)gridDim.x * ADAM_THREADS;
    for (size_t i = (size_t)blockIdx.x * ADAM_THREADS + threadIdx.x; i < n; i += stride) {
        if (VEC) {
            f32x4* p4 = reinterpret_cast<f32x4*>(p);
            f32x4* m4 = reinterpret_cast<f32x4*>(m);
            f32x4* v4 = reinterpret_cast<f32x4*>(v);
            f32x4* e4 = reinterpret_cast<f32x4*>(ema);
            f32x4 w = p4[i];
            const f32x4 gv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g) + i);
            f32x4 mv = __builtin_nontemporal_load(m4 + i);
            f32x4 vv = __builtin_nontemporal_load(v4 + i);
            f32x4 e = {0.f, 0.f, 0.f, 0.f};
            if (EMA) e = __builtin_nontemporal_load(e4 + i);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float wk = w[k], mk = mv[k], vk = vv[k], ek = e[k];
                adam_element<EMA>(wk, gv[k], mk, vk, ek, s);
                w[k] = wk;
                mv[k] = mk;
                vv[k] = vk;
                e[k] = ek;
            }
            __builtin_nontemporal_store(mv, m4 + i);
            __builtin_nontemporal_store(vv, v4 + i);
            p4[i] = w;
            if (EMA) __builtin_nontemporal_store(e, e4 + i);
        } else {
            float w = p[i], mk = m[i], vk = v[i], e = EMA ? ema[i] : 0.f;
            adam_element<EMA>(w, g[i], mk, vk, e, s);
            m[i] = mk;
            v[i] = vk;
            p[i] = w;
            if (EMA) ema[i] = e;
        }
    }
}

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }
inline bool beta_ok(double b) { return b >= 0.0 && b < 1.0; }           // (NaN fails both)

}  // namespace

extern "C" int ssd_adam_advance(void* state, double beta1, double beta2, const int* skip_dev, void* stream) {
    if (!state) return SSD_ERR_NULL;
    if (!beta_ok(beta1) || !beta_ok(beta2)) return SSD_ERR_BAD_SHAPE;
    if (!aligned8(state) || !aligned4(skip_dev)) return SSD_ERR_ALIGN;
    hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, static_cast<double*>(state), beta1, beta2, skip_dev);
    SSD_CHECK_LAUNCH();
    return SSD_OK;
}

extern "C" int ssd_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, size_t n, double lr,
                             const float* lr_dev, const float* ema_w_dev, const void* state, double beta1, double beta2, double eps,
                             double weight_decay, int decoupled, const float* grad_scale_dev, const int* skip_dev, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || !state || (ema && !ema_w_dev)) return SSD_ERR_NULL;
    if (!beta_ok(beta1) || !beta_ok(beta2) || !(eps >= 0.0) || !(weight_decay >= 0.0) || (!lr_dev && !(lr >= 0.0))) return SSD_ERR_BAD_SHAPE;
    if (!aligned4(param) || !aligned4(grad) || !aligned4(exp_avg) || !aligned4(exp_avg_sq) || !aligned4(ema) || !aligned4(lr_dev) ||
        !aligned4(ema_w_dev) || !aligned4(grad_scale_dev) || !aligned4(skip_dev) || !aligned8(state))
        return SSD_ERR_ALIGN;
    if (n == 0) return SSD_OK;
    const bool vec = (n & 3) == 0 && ssd_aligned16(param) && ssd_aligned16(grad) && ssd_aligned16(exp_avg) && ssd_aligned16(exp_avg_sq) &&
                     ssd_aligned16(ema);
    const size_t units = vec ? n / 4 : n;
    const dim3 grid(adam_blocks(units)), block(ADAM_THREADS);
    hipStream_t st = (hipStream_t)stream;
    AdamScalars s = {};
    s.omb1 = (float)(1.0 - beta1);
    s.omb2 = (float)(1.0 - beta2);
    s.b2 = (float)beta2;
    s.eps = (float)eps;
    s.wd = (float)weight_decay;
    s.decoupled = decoupled != 0;
    s.has_wd = weight_decay != 0.0;
    const double* st64 = static_cast<const double*>(state);
#define SSD_ADAM_LAUNCH(V, E)                                                                                                           \
    hipLaunchKernelGGL((adam_kernel<V, E>), grid, block, 0, st, param, grad, exp_avg, exp_avg_sq, ema, units, lr, lr_dev, ema_w_dev, st64, \
                       s, weight_decay, grad_scale_dev, skip_dev)
    if (vec) {
        if (ema) SSD_ADAM_LAUNCH(true, true);
        else SSD_ADAM_LAUNCH(true, false);
    } else {
        if (ema) SSD_ADAM_LAUNCH(false, true);
        else SSD_ADAM_LAUNCH(false, false);
    }
#undef SSD_ADAM_LAUNCH
    SSD_CHECK_LAUNCH();
    return SSD_OK;
}
