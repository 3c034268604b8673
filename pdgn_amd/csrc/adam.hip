// adam.hip -- the Adam update of a whole parameter list in ONE launch with thousands of workgroups.
//
// The reference steps five torch.optim.Adam optimisers per iteration (models/PDGNet_v2.py:121-125, 186-226, 256: lr 1e-4,
// betas (0.5, 0.999), no weight decay, no amsgrad).  torch's fused multi-tensor kernel walks a list in chunks of 64 K elements --
// 194 workgroups for the generator's 12.7 M parameters, in five launches: 230 us at the end of every iteration, on the chain the next
// iteration waits for (1.5 TB/s of the 355 MB it moves).  Here a workgroup takes ADAM_CHUNK elements of one tensor of the list
// (found by bisection in a table of first chunks); the arithmetic is torch's (ATen/native/cuda/fused_adam_utils.cuh, the
// non-amsgrad, non-maximize, weight_decay = 0 case):
//     m <- beta1 m + (1 - beta1) g;  v <- beta2 v + (1 - beta2) g g;        (in fp64, as torch's double betas make them)
//     p <- p - (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
// with the bias corrections in fp64 from the step count t that torch keeps as a device tensor (read here, incremented by the caller).
#include "common.h"
#include <type_traits>

#define ADAM_THREADS 256
#define ADAM_CHUNK 4096            // elements per workgroup: four float4 per thread
#define ADAM_MAXT 72               // tensors per launch: their pointers travel in the kernel arguments (3.5 KB of the 4 KB there are)

#define ADAM_EMA_MAXT 64           // ... with the averages' pointers beside them: 52 bytes per tensor, 3.4 KB of arguments (72 would be 3.8 KB,
                                   // which leaves the runtime's hidden arguments less room than they take)

struct AdamArgs {                  // by value: a recorded iteration (csrc/replay.hip) re-issues the launch with the same pointers
    float *p[ADAM_MAXT];
    const float *g[ADAM_MAXT];
    float *m[ADAM_MAXT];
    float *v[ADAM_MAXT];
    long long n[ADAM_MAXT];        // elements
    int chunk0[ADAM_MAXT];         // index of the tensor's first chunk among this launch's chunks
    int ntensors;
};

struct AdamEmaArgs {               // the same table with the list of averages (pdgn_adam_ema_multi)
    float *p[ADAM_EMA_MAXT];
    const float *g[ADAM_EMA_MAXT];
    float *m[ADAM_EMA_MAXT];
    float *v[ADAM_EMA_MAXT];
    float *e[ADAM_EMA_MAXT];
    long long n[ADAM_EMA_MAXT];
    int chunk0[ADAM_EMA_MAXT];
    int ntensors;
};
static_assert(sizeof(AdamArgs) + 48 <= 3584 && sizeof(AdamEmaArgs) + 56 <= 3584, "pointer tables: 3.5 KB of the 4 KB of kernel arguments");
static_assert(sizeof(AdamArgs) + 56 <= 3584 && sizeof(AdamEmaArgs) + 64 <= 3584, "... with the schedule's pointer behind them");

// ---- the generator's averaged copy (an exponential moving average of the parameters, Yazici et al. 2019), one expression for the
// fused launch, the stand-alone launch and the host mirror of the tests: with t the step count of THIS update,
//     d_t = min(ema_decay, (1 + t) / (10 + t))   in fp64 (the usual warm-up, from the device-side counter: a replayed launch needs
//                                                 no host value);      omd = (float)(1 - d_t)
//     e <- e + omd * (p_new - e)                  three separately rounded fp32 operations, never an FMA
__device__ __forceinline__ float ema_one_minus_decay(double ema_decay, const float *step) {
    const double t = (double)step[0];
    const double warm = (1.0 + t) / (10.0 + t);
    return (float)(1.0 - (ema_decay < warm ? ema_decay : warm));
}
__device__ __forceinline__ void ema_one(float &e, float p, float omd) { e = __fadd_rn(e, __fmul_rn(omd, __fsub_rn(p, e))); }

// ---- the learning-rate schedule: a piecewise-linear factor f(t) of the step count t of THIS update, from a table of
// PDGN_LR_TABLE_DOUBLES fp64 words in device memory (include/pdgn_hip.h states the layout and these expressions; tests/lr_mirror.py
// restates them in numpy and demands equal bits): tab[0] = n knots, tab[1 + 2i] = t_i, tab[2 + 2i] = f_i.
//     f = f_0 for t <= t_0;  f = f_{n-1} for t >= t_{n-1};  else, with the first i (scanned from 0) for which t < t_{i+1}:
//     f = dadd(f_i, dmul(dsub(f_{i+1}, f_i), ddiv(dsub(t, t_i), dsub(t_{i+1}, t_i))))      every operation rounded on its own
// A malformed table (n no integer in 1 .. 16, some t_{i+1} <= t_i or NaN) gives f_0; no word past tab[2n] is ever read, and none
// past tab[2] for an n out of range.  The index is uniform and the table read-only: the loads are scalar ones.
__device__ __forceinline__ double lr_factor(const double *__restrict__ tab, double t) {
    const double nd = tab[0], f0 = tab[2];
    if (!(nd >= 1.0 && nd <= (double)PDGN_LR_MAX_KNOTS)) return f0;
    const int n = (int)nd;
    if ((double)n != nd) return f0;
    int seg = -1;
    for (int i = 0; i + 1 < n; ++i) {
        if (!(tab[3 + 2 * i] > tab[1 + 2 * i])) return f0;
        if (seg < 0 && t < tab[3 + 2 * i]) seg = i;
    }
    if (t <= tab[1]) return f0;
    if (seg < 0) return tab[2 * n];                              // t >= t_{n-1}
    const double ti = tab[1 + 2 * seg], fi = tab[2 + 2 * seg], tj = tab[3 + 2 * seg], fj = tab[4 + 2 * seg];
    return __dadd_rn(fi, __dmul_rn(__dsub_rn(fj, fi), __ddiv_rn(__dsub_rn(t, ti), __dsub_rn(tj, ti))));
}

// One chunk of one tensor.  EMA = false is pdgn_adam_multi's kernel; EMA = true adds the average E to the same walk (one more load
// in front of the stores, one more store behind them): the Adam arithmetic is this one text for both.  GUARD = true reads the
// network's guard record first (written by pdgn_gradnorm_multi on the same stream): applied == 0 leaves before anything is touched,
// otherwise the gradient that enters the arithmetic is fmul(g, coef), rounded on its own; g itself is never written.  SCHED = true
// multiplies lr by the schedule's factor at this update's t (lr_factor above), once per workgroup where step_size is formed.
template <bool EMA, bool GUARD, bool SCHED = false, class Args>
__device__ __forceinline__ void adam_chunk(const Args &a, double lr, double beta1d, double beta2d, double eps, double ema_decay,
                                           const float *__restrict__ step, const pdgn_guard_record *__restrict__ guard = nullptr,
                                           const double *__restrict__ sched = nullptr) {
    __shared__ float sc[EMA ? 3 : 2];
    float coef = 1.f;
    if constexpr (GUARD) {
        if (guard->applied == 0.f) return;                       // the whole grid takes the same way: the record is complete before the launch
        coef = guard->coef;
    }
    // the chunk's tensor: the last one whose first chunk is <= this chunk
    int lo = 0, hi = a.ntensors - 1;
    const int c = blockIdx.x;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.chunk0[mid] <= c) lo = mid; else hi = mid - 1;
    }
    float *const P = a.p[lo], *const M = a.m[lo], *const V = a.v[lo];
    const float *const G = a.g[lo];
    float *E = nullptr;
    if constexpr (EMA) E = a.e[lo];
    const long long n = a.n[lo];
    if (threadIdx.x == 0) {
        // torch: the two bias corrections in fp64, handed to the arithmetic as floats; step_size = lr (double) / that float
        const double t = (double)step[0];
        const float bc1 = (float)(1.0 - pow(beta1d, t));
        if constexpr (SCHED) lr = __dmul_rn(lr, lr_factor(sched, t));
        sc[0] = (float)(lr / (double)bc1);
        sc[1] = (float)sqrt(1.0 - pow(beta2d, t));
        if constexpr (EMA) sc[2] = ema_one_minus_decay(ema_decay, step);
    }
    __syncthreads();
    const float step_size = sc[0], bc2s = sc[1];
    float omd = 0.f;
    if constexpr (EMA) omd = sc[2];
    const double epsd = (double)eps, w1 = 1.0 - beta1d, w2 = 1.0 - beta2d;
    const long long i0 = (long long)(c - a.chunk0[lo]) * ADAM_CHUNK;
    const bool vec = ((((uintptr_t)P | (uintptr_t)G | (uintptr_t)M | (uintptr_t)V | (uintptr_t)E) & 15) == 0);
    // torch's expressions with torch's types (lr, betas, eps are doubles there: the moment updates are evaluated in fp64 and rounded
    // once, 1 - beta is 1 - the DOUBLE beta): the results are torch's bits, not merely close to them
    auto one = [&](float &p, float g, float &m, float &v) {
        if constexpr (GUARD) g = __fmul_rn(g, coef);
        m = (float)(beta1d * (double)m + w1 * (double)g);
        v = (float)(beta2d * (double)v + (w2 * (double)g) * (double)g);
        const float denom = (float)((double)(sqrtf(v) / bc2s) + epsd);
        p -= step_size * m / denom;
    };
    if (vec) {
        // all loads of the chunk first (the stores below may alias them as far as the compiler knows: interleaved, every float4
        // group waited for the one before), then the arithmetic, then the stores
        constexpr int NU = ADAM_CHUNK / (4 * ADAM_THREADS);
        float4 p4[NU], g4[NU], m4[NU], v4[NU], e4[EMA ? NU : 1];
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const long long i = i0 + 4LL * (threadIdx.x + u * ADAM_THREADS);
            if (i + 3 < n) {
                p4[u] = *reinterpret_cast<const float4 *>(P + i);
                g4[u] = *reinterpret_cast<const float4 *>(G + i);
                m4[u] = *reinterpret_cast<const float4 *>(M + i);
                v4[u] = *reinterpret_cast<const float4 *>(V + i);
                if constexpr (EMA) e4[u] = *reinterpret_cast<const float4 *>(E + i);
            }
        }
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const long long i = i0 + 4LL * (threadIdx.x + u * ADAM_THREADS);
            if (i + 3 < n) {
                one(p4[u].x, g4[u].x, m4[u].x, v4[u].x); one(p4[u].y, g4[u].y, m4[u].y, v4[u].y);
                one(p4[u].z, g4[u].z, m4[u].z, v4[u].z); one(p4[u].w, g4[u].w, m4[u].w, v4[u].w);
                *reinterpret_cast<float4 *>(P + i) = p4[u];
                *reinterpret_cast<float4 *>(M + i) = m4[u];
                *reinterpret_cast<float4 *>(V + i) = v4[u];
                if constexpr (EMA) {
                    ema_one(e4[u].x, p4[u].x, omd); ema_one(e4[u].y, p4[u].y, omd);
                    ema_one(e4[u].z, p4[u].z, omd); ema_one(e4[u].w, p4[u].w, omd);
                    *reinterpret_cast<float4 *>(E + i) = e4[u];
                }
            } else {
                for (long long j = i; j < n && j < i + 4; ++j) {
                    one(P[j], G[j], M[j], V[j]);
                    if constexpr (EMA) ema_one(E[j], P[j], omd);
                }
            }
        }
    } else {
        for (long long i = i0 + threadIdx.x; i < n && i < i0 + ADAM_CHUNK; i += ADAM_THREADS) {
            one(P[i], G[i], M[i], V[i]);
            if constexpr (EMA) ema_one(E[i], P[i], omd);
        }
    }
}

// The four launches with a schedule (pdgn_adam_sched_multi).  Defined in front of the kernels they are variants of, as the guard's
// are in front of ema_multi_kernel: tools/isa_diff.py compares a kernel with its trailing padding, which depends on what follows it.
__global__ __launch_bounds__(ADAM_THREADS) void adam_sched_multi_kernel(const AdamArgs a, double lr, double beta1d, double beta2d, double eps,
                                                                        const float *__restrict__ step, const double *__restrict__ sched) {
    adam_chunk<false, false, true>(a, lr, beta1d, beta2d, eps, 0.0, step, nullptr, sched);
}

__global__ __launch_bounds__(ADAM_THREADS) void adam_ema_sched_multi_kernel(const AdamEmaArgs a, double lr, double beta1d, double beta2d,
                                                                            double eps, double ema_decay, const float *__restrict__ step,
                                                                            const double *__restrict__ sched) {
    adam_chunk<true, false, true>(a, lr, beta1d, beta2d, eps, ema_decay, step, nullptr, sched);
}

__global__ __launch_bounds__(ADAM_THREADS) void adam_guard_sched_multi_kernel(const AdamArgs a, double lr, double beta1d, double beta2d,
                                                                              double eps, const float *__restrict__ step,
                                                                              const pdgn_guard_record *__restrict__ guard,
                                                                              const double *__restrict__ sched) {
    adam_chunk<false, true, true>(a, lr, beta1d, beta2d, eps, 0.0, step, guard, sched);
}

__global__ __launch_bounds__(ADAM_THREADS) void adam_ema_guard_sched_multi_kernel(const AdamEmaArgs a, double lr, double beta1d, double beta2d,
                                                                                  double eps, double ema_decay, const float *__restrict__ step,
                                                                                  const pdgn_guard_record *__restrict__ guard,
                                                                                  const double *__restrict__ sched) {
    adam_chunk<true, true, true>(a, lr, beta1d, beta2d, eps, ema_decay, step, guard, sched);
}

// f and lr_eff of the update that is ABOUT to happen, by one thread: t = fadd(step[0], guard ? guard->applied : 1) -- the fp32 sum the
// caller's counter update forms -- out2 = {f, dmul(lr, f)} and out_lr32 = (float)out2[1]: what the routes through torch hand its
// kernel as a tensor lr.
__global__ void lr_eval_kernel(const double *__restrict__ sched, double lr, const float *__restrict__ step,
                               const pdgn_guard_record *__restrict__ guard, double *__restrict__ out2, float *__restrict__ out_lr32) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const double t = (double)__fadd_rn(step[0], guard ? guard->applied : 1.f);
    const double f = lr_factor(sched, t), lr_eff = __dmul_rn(lr, f);
    out2[0] = f;
    out2[1] = lr_eff;
    out_lr32[0] = (float)lr_eff;
}

__global__ __launch_bounds__(ADAM_THREADS) void adam_multi_kernel(const AdamArgs a, double lr, double beta1d, double beta2d, double eps,
                                                                  const float *__restrict__ step) {
    adam_chunk<false, false>(a, lr, beta1d, beta2d, eps, 0.0, step);
}

__global__ __launch_bounds__(ADAM_THREADS) void adam_ema_multi_kernel(const AdamEmaArgs a, double lr, double beta1d, double beta2d, double eps,
                                                                      double ema_decay, const float *__restrict__ step) {
    adam_chunk<true, false>(a, lr, beta1d, beta2d, eps, ema_decay, step);
}

__global__ __launch_bounds__(ADAM_THREADS) void adam_guard_multi_kernel(const AdamArgs a, double lr, double beta1d, double beta2d, double eps,
                                                                        const float *__restrict__ step,
                                                                        const pdgn_guard_record *__restrict__ guard) {
    adam_chunk<false, true>(a, lr, beta1d, beta2d, eps, 0.0, step, guard);
}

__global__ __launch_bounds__(ADAM_THREADS) void adam_ema_guard_multi_kernel(const AdamEmaArgs a, double lr, double beta1d, double beta2d,
                                                                            double eps, double ema_decay, const float *__restrict__ step,
                                                                            const pdgn_guard_record *__restrict__ guard) {
    adam_chunk<true, true>(a, lr, beta1d, beta2d, eps, ema_decay, step, guard);
}

// ---- the host side all the multi-tensor launches of this file share.  A list is walked MAXT tensors per launch (MAXT: the length of
// the argument struct's columns); every launch's chunk count is checked before the first launch.
// Chunks of the whole list, or -1 where one launch's MAXT tensors have more than 2^30 - 1 of them (every n[i] >= 1 is the caller's to check).
static long long list_chunks(int ntensors, const long long *n, int maxt) {
    long long total = 0;
    for (int t0 = 0; t0 < ntensors; t0 += maxt) {
        long long chunks = 0;
        for (int i = t0; i < ntensors && i < t0 + maxt; ++i) chunks += (n[i] + ADAM_CHUNK - 1) / ADAM_CHUNK;
        if (chunks > 0x3fffffffLL) return -1;
        total += chunks;
    }
    return total;
}

// Per launch: n[] and chunk0[] of an Args filled, its tail padded (null pointers, 0 elements, a first chunk no workgroup reaches), then
// launch(a, t0, chunks) sets the pointer columns a.x[i] <- x[t0 + i] for i < a.ntensors and launches `chunks` workgroups.  PDGN_ERR_INVALID
// before anything is launched, else 0: the launches are issued, their status is the caller's to ask for.
template <class Args, class Launch>
static int for_each_launch(int ntensors, const long long *n, Launch launch) {
    constexpr int MAXT = (int)(sizeof(Args::n) / sizeof(long long));
    if (list_chunks(ntensors, n, MAXT) < 0) return PDGN_ERR_INVALID;
    for (int t0 = 0; t0 < ntensors; t0 += MAXT) {
        Args a = {};
        a.ntensors = ntensors - t0 < MAXT ? ntensors - t0 : MAXT;
        long long chunks = 0;
        for (int i = 0; i < a.ntensors; ++i) {
            a.n[i] = n[t0 + i];
            a.chunk0[i] = (int)chunks;
            chunks += (n[t0 + i] + ADAM_CHUNK - 1) / ADAM_CHUNK;
        }
        for (int i = a.ntensors; i < MAXT; ++i) a.chunk0[i] = 0x7fffffff;
        launch(a, t0, (unsigned)chunks);
    }
    return 0;
}

// One Adam step of `ntensors` fp32 tensors (p, g, m, v: HOST arrays of device pointers; n: their element counts), in
// ceil(ntensors / 72) launches of one workgroup per 4096 elements.  step (device): the step count t >= 1 of THIS update as one
// float (torch's `state["step"]` after its increment).  Replaces torch._fused_adam_ / optimizer.step() of the reference's five Adam
// optimisers (models/PDGNet_v2.py:121-125, 186-226, 256) for lists without weight decay, amsgrad or maximize.
// (a guard record is read with dword loads: the address the guarded entry points refuse.  `guard` null = the unguarded kernel.)
static bool guard_misplaced(const pdgn_guard_record *guard) { return ((uintptr_t)guard & 3) != 0; }
// (a schedule is read with 8-byte loads.  `sched` null = the kernel without one.)
static bool sched_misplaced(const double *sched) { return ((uintptr_t)sched & 7) != 0; }

// Args = AdamEmaArgs: the averages e (HOST array of device pointers) updated in the same launches, ceil(ntensors / 64) of them: p, m, v
// are pdgn_adam_multi's bits; e <- e + (1 - d_t) (p_new - e) as written at ema_one_minus_decay above.  No reference counterpart (the
// reference keeps no averaged generator).  Args = AdamArgs: e and ema_decay are not read.
template <class Args>
static int adam_multi_launch(int ntensors, void *const *p, const void *const *g, void *const *m, void *const *v, void *const *e,
                             const long long *n, double lr, double beta1, double beta2, double eps, double ema_decay, const float *step,
                             const pdgn_guard_record *guard, const double *sched, pdgn_stream_t stream) {
    constexpr bool EMA = std::is_same<Args, AdamEmaArgs>::value;
    if (ntensors < 1 || !p || !g || !m || !v || (EMA && !e) || !n || !step || !(lr >= 0.) || !(beta1 >= 0. && beta1 < 1.) ||
        !(beta2 >= 0. && beta2 < 1.) || !(eps >= 0.) || (EMA && !(ema_decay >= 0. && ema_decay < 1.)))
        return PDGN_ERR_INVALID;
    for (int i = 0; i < ntensors; ++i)
        if (!p[i] || !g[i] || !m[i] || !v[i] || (EMA && !e[i]) || n[i] < 1 ||
            (((uintptr_t)p[i] | (uintptr_t)g[i] | (uintptr_t)m[i] | (uintptr_t)v[i] | (EMA ? (uintptr_t)e[i] : 0)) & 3))
            return PDGN_ERR_INVALID;
    if (guard_misplaced(guard) || sched_misplaced(sched)) return PDGN_ERR_INVALID;
    const int rc = for_each_launch<Args>(ntensors, n, [&](Args &a, int t0, unsigned chunks) {
        for (int i = 0; i < a.ntensors; ++i) {
            a.p[i] = (float *)p[t0 + i]; a.g[i] = (const float *)g[t0 + i]; a.m[i] = (float *)m[t0 + i]; a.v[i] = (float *)v[t0 + i];
            if constexpr (EMA) a.e[i] = (float *)e[t0 + i];
        }
        const dim3 grid(chunks), block(ADAM_THREADS);
        const hipStream_t s = (hipStream_t)stream;
        if constexpr (EMA) {
            if (sched && guard) hipLaunchKernelGGL(adam_ema_guard_sched_multi_kernel, grid, block, 0, s, a, lr, beta1, beta2, eps, ema_decay, step, guard, sched);
            else if (sched) hipLaunchKernelGGL(adam_ema_sched_multi_kernel, grid, block, 0, s, a, lr, beta1, beta2, eps, ema_decay, step, sched);
            else if (guard) hipLaunchKernelGGL(adam_ema_guard_multi_kernel, grid, block, 0, s, a, lr, beta1, beta2, eps, ema_decay, step, guard);
            else hipLaunchKernelGGL(adam_ema_multi_kernel, grid, block, 0, s, a, lr, beta1, beta2, eps, ema_decay, step);
        } else {
            if (sched && guard) hipLaunchKernelGGL(adam_guard_sched_multi_kernel, grid, block, 0, s, a, lr, beta1, beta2, eps, step, guard, sched);
            else if (sched) hipLaunchKernelGGL(adam_sched_multi_kernel, grid, block, 0, s, a, lr, beta1, beta2, eps, step, sched);
            else if (guard) hipLaunchKernelGGL(adam_guard_multi_kernel, grid, block, 0, s, a, lr, beta1, beta2, eps, step, guard);
            else hipLaunchKernelGGL(adam_multi_kernel, grid, block, 0, s, a, lr, beta1, beta2, eps, step);
        }
    });
    return rc ? rc : pdgn_launch_status();
}

extern "C" int pdgn_adam_multi(int ntensors, void *const *p, const void *const *g, void *const *m, void *const *v, const long long *n,
                               double lr, double beta1, double beta2, double eps, const float *step, pdgn_stream_t stream) {
    return adam_multi_launch<AdamArgs>(ntensors, p, g, m, v, nullptr, n, lr, beta1, beta2, eps, 0., step, nullptr, nullptr, stream);
}

// pdgn_adam_multi with the averages (adam_multi_launch<AdamEmaArgs> above).
extern "C" int pdgn_adam_ema_multi(int ntensors, void *const *p, const void *const *g, void *const *m, void *const *v, void *const *e,
                                   const long long *n, double lr, double beta1, double beta2, double eps, double ema_decay,
                                   const float *step, pdgn_stream_t stream) {
    return adam_multi_launch<AdamEmaArgs>(ntensors, p, g, m, v, e, n, lr, beta1, beta2, eps, ema_decay, step, nullptr, nullptr, stream);
}

// The two launches above behind a gradient guard (pdgn_gradnorm_multi below, on the same stream in front of them): every workgroup
// reads the network's record; applied == 0 leaves p, m, v, e as they are, otherwise the gradient in the arithmetic is fmul(g, coef).
// With coef == 1 the bits are the unguarded launches'.  guard: the record (device), never null here.
extern "C" int pdgn_adam_guard_multi(int ntensors, void *const *p, const void *const *g, void *const *m, void *const *v, const long long *n,
                                     double lr, double beta1, double beta2, double eps, const float *step, const pdgn_guard_record *guard,
                                     pdgn_stream_t stream) {
    if (!guard) return PDGN_ERR_INVALID;
    return adam_multi_launch<AdamArgs>(ntensors, p, g, m, v, nullptr, n, lr, beta1, beta2, eps, 0., step, guard, nullptr, stream);
}

extern "C" int pdgn_adam_ema_guard_multi(int ntensors, void *const *p, const void *const *g, void *const *m, void *const *v, void *const *e,
                                         const long long *n, double lr, double beta1, double beta2, double eps, double ema_decay,
                                         const float *step, const pdgn_guard_record *guard, pdgn_stream_t stream) {
    if (!guard) return PDGN_ERR_INVALID;
    return adam_multi_launch<AdamEmaArgs>(ntensors, p, g, m, v, e, n, lr, beta1, beta2, eps, ema_decay, step, guard, nullptr, stream);
}

// The four launches above with a learning-rate schedule (lr_factor at the top of this file): the rate in the arithmetic is
// dmul(lr, f(t)) with t = step[0], everything else is the entry point that e and guard select -- e null: pdgn_adam_multi /
// pdgn_adam_guard_multi (ema_decay is not read), else pdgn_adam_ema_multi / pdgn_adam_ema_guard_multi; guard null: unguarded.
// sched (device, 8-byte aligned, PDGN_LR_TABLE_DOUBLES doubles): never null here.  No reference counterpart.
extern "C" int pdgn_adam_sched_multi(int ntensors, void *const *p, const void *const *g, void *const *m, void *const *v, void *const *e,
                                     const long long *n, double lr, double beta1, double beta2, double eps, double ema_decay,
                                     const float *step, const pdgn_guard_record *guard, const double *sched, pdgn_stream_t stream) {
    if (!sched) return PDGN_ERR_INVALID;
    if (!e) return adam_multi_launch<AdamArgs>(ntensors, p, g, m, v, nullptr, n, lr, beta1, beta2, eps, 0., step, guard, sched, stream);
    return adam_multi_launch<AdamEmaArgs>(ntensors, p, g, m, v, e, n, lr, beta1, beta2, eps, ema_decay, step, guard, sched, stream);
}

// out2[0..1] <- {f, lr_eff}, out_lr32[0] <- (float)lr_eff of the update about to happen (lr_eval_kernel above): one thread, on `stream`.
extern "C" int pdgn_lr_eval(const double *sched, double lr, const float *step, const pdgn_guard_record *guard, double *out2,
                            float *out_lr32, pdgn_stream_t stream) {
    if (!sched || sched_misplaced(sched) || !(lr >= 0.) || !step || ((uintptr_t)step & 3) || guard_misplaced(guard) || !out2 ||
        ((uintptr_t)out2 & 7) || !out_lr32 || ((uintptr_t)out_lr32 & 3))
        return PDGN_ERR_INVALID;
    hipLaunchKernelGGL(lr_eval_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, sched, lr, step, guard, out2, out_lr32);
    return pdgn_launch_status();
}

// ---- the same walk for a plain copy: dst[i] <- src[i] for a list of fp32 tensors (the pack of a network's fresh gradients into the
// flat all-reduce buffer, optim.FlatGrads: torch._foreach_copy_ takes 82 us for the generator's 160 tensors / 50.8 MB)
#define COPY_MAXT 128               // tensors per launch (28 bytes of arguments each)
struct CopyArgs {
    float *d[COPY_MAXT];
    const float *s[COPY_MAXT];
    long long n[COPY_MAXT];
    int chunk0[COPY_MAXT];
    int ntensors;
};

__global__ __launch_bounds__(ADAM_THREADS) void copy_multi_kernel(const CopyArgs a) {
    int lo = 0, hi = a.ntensors - 1;
    const int c = blockIdx.x;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.chunk0[mid] <= c) lo = mid; else hi = mid - 1;
    }
    float *const D = a.d[lo];
    const float *const S = a.s[lo];
    const long long n = a.n[lo], i0 = (long long)(c - a.chunk0[lo]) * ADAM_CHUNK;
    if (((((uintptr_t)D | (uintptr_t)S) & 15) == 0)) {
        constexpr int NU = ADAM_CHUNK / (4 * ADAM_THREADS);
        float4 v[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const long long i = i0 + 4LL * (threadIdx.x + u * ADAM_THREADS);
            if (i + 3 < n) v[u] = *reinterpret_cast<const float4 *>(S + i);
        }
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const long long i = i0 + 4LL * (threadIdx.x + u * ADAM_THREADS);
            if (i + 3 < n) *reinterpret_cast<float4 *>(D + i) = v[u];
            else for (long long j = i; j < n && j < i + 4; ++j) D[j] = S[j];
        }
    } else {
        for (long long i = i0 + threadIdx.x; i < n && i < i0 + ADAM_CHUNK; i += ADAM_THREADS) D[i] = S[i];
    }
}

// dst[i] (n[i] floats) <- src[i] for ntensors fp32 tensors (HOST arrays of device pointers, 4-byte aligned; 16-byte aligned pairs
// take the vector path), in ceil(ntensors / 128) launches.  Replaces torch._foreach_copy_ where a network's gradients are packed
// into one buffer for the all-reduce (the DataParallel gradient reduction of models/PDGNet_v2.py:101-105).
extern "C" int pdgn_copy_multi(int ntensors, void *const *dst, const void *const *src, const long long *n, pdgn_stream_t stream) {
    if (ntensors < 1 || !dst || !src || !n) return PDGN_ERR_INVALID;
    for (int i = 0; i < ntensors; ++i)
        if (!dst[i] || !src[i] || n[i] < 1 || (((uintptr_t)dst[i] | (uintptr_t)src[i]) & 3)) return PDGN_ERR_INVALID;
    const int rc = for_each_launch<CopyArgs>(ntensors, n, [&](CopyArgs &a, int t0, unsigned chunks) {
        for (int i = 0; i < a.ntensors; ++i) { a.d[i] = (float *)dst[t0 + i]; a.s[i] = (const float *)src[t0 + i]; }
        hipLaunchKernelGGL(copy_multi_kernel, dim3(chunks), dim3(ADAM_THREADS), 0, (hipStream_t)stream, a);
    });
    return rc ? rc : pdgn_launch_status();
}

// ---- the same walk for the average alone: e[i] <- e[i] + (1 - d_t) (p[i] - e[i]), where the optimizer step in front of it was not
// pdgn_adam_ema_multi (the optimizer's first, ordinary step; torch's fused kernel).  ema_one_minus_decay / ema_one are the fused
// launch's: the same bits.
struct EmaArgs {
    float *e[COPY_MAXT];
    const float *p[COPY_MAXT];
    long long n[COPY_MAXT];
    int chunk0[COPY_MAXT];
    int ntensors;
};

// ---- the gradient guard: the 2-norm of a whole list of fp32 tensors, on the device, in two launches and a fixed order of additions
// (no float atomics, no last-block-done counter: the same bytes give the same bits).
//   launch 1 (one workgroup per 4096-element chunk, the walk of the kernels above): every thread squares its 16 elements IN FP64 and
//     adds them in element order, the wave adds its 64 lanes by a shuffle tree, thread 0 adds the four waves' sums from LDS in wave
//     order; one fp64 partial per chunk goes to the caller's workspace.  A thread's elements are the same 16 on the vector and the
//     scalar path, so the bits do not depend on the tensors' alignment either.
//   launch 2 (one workgroup): the partials through LDS, added by thread 0 in index order; the record is written there.
// fp64 squares of fp32 values neither overflow nor vanish (|g| <= 3.4e38: g^2 <= 1.2e77; the smallest denormal squared is 2e-90),
// so the total is non-finite exactly when an element is NaN or +-Inf.
struct GradArgs {
    const float *g[COPY_MAXT];
    long long n[COPY_MAXT];
    int chunk0[COPY_MAXT];
    int ntensors;
};
#define GUARD_TILE 2048             // partials per pass of the finalising workgroup through LDS (16 KB)

__global__ __launch_bounds__(ADAM_THREADS) void gradnorm_partial_kernel(const GradArgs a, double *__restrict__ partial) {
    __shared__ double sw[ADAM_THREADS / 64];
    int lo = 0, hi = a.ntensors - 1;
    const int c = blockIdx.x;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.chunk0[mid] <= c) lo = mid; else hi = mid - 1;
    }
    const float *const G = a.g[lo];
    const long long n = a.n[lo], i0 = (long long)(c - a.chunk0[lo]) * ADAM_CHUNK;
    constexpr int NU = ADAM_CHUNK / (4 * ADAM_THREADS);
    const bool vec = (((uintptr_t)G & 15) == 0);
    float4 g4[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const long long i = i0 + 4LL * (threadIdx.x + u * ADAM_THREADS);
        g4[u] = make_float4(0.f, 0.f, 0.f, 0.f);                 // past the end: zeros, whose squares change no sum
        if (vec && i + 3 < n) {
            g4[u] = *reinterpret_cast<const float4 *>(G + i);
        } else {
            if (i < n) g4[u].x = G[i];
            if (i + 1 < n) g4[u].y = G[i + 1];
            if (i + 2 < n) g4[u].z = G[i + 2];
            if (i + 3 < n) g4[u].w = G[i + 3];
        }
    }
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        s += (double)g4[u].x * (double)g4[u].x; s += (double)g4[u].y * (double)g4[u].y;
        s += (double)g4[u].z * (double)g4[u].z; s += (double)g4[u].w * (double)g4[u].w;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = sw[0];
#pragma unroll
        for (int w = 1; w < ADAM_THREADS / 64; ++w) t += sw[w];
        partial[c] = t;
    }
}

__global__ __launch_bounds__(ADAM_THREADS) void gradnorm_final_kernel(const double *__restrict__ partial, long long nparts, double max_norm,
                                                                      pdgn_guard_record *__restrict__ rec) {
    __shared__ double tile[GUARD_TILE];
    double total = 0.0;
    for (long long base = 0; base < nparts; base += GUARD_TILE) {
        const int m = (int)(nparts - base < GUARD_TILE ? nparts - base : GUARD_TILE);
        for (int i = threadIdx.x; i < m; i += ADAM_THREADS) tile[i] = partial[base + i];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < m; ++i) total += tile[i];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const bool finite = isfinite(total);
        const double norm64 = sqrt(total);
        float coef = 1.f;                                        // no clipping: max_norm <= 0 or infinite; nothing to clip: a skipped update
        if (finite && max_norm > 0. && isfinite(max_norm)) {
            const double r = max_norm / (norm64 + 1e-6);
            coef = (float)(r < 1.0 ? r : 1.0);
        }
        rec->norm = (float)norm64;
        rec->coef = coef;
        rec->applied = finite ? 1.f : 0.f;
        rec->found_inf = finite ? 0.f : 1.f;
        rec->n_applied += finite ? 1u : 0u;
        rec->n_skipped += finite ? 0u : 1u;
    }
}

// ema_multi_kernel (below) behind a guard record: applied == 0 (the update in front of this launch was skipped) leaves e as it is.
// Its own copy of the text, not a switch in that kernel, and placed -- like the guard's other kernels -- in front of it: the unguarded
// kernel's machine code is pinned (tools/isa_diff.py compares it with its padding, which depends on what follows it in the object,
// and the compiler numbers the registers of an inlined shared body differently).
__global__ __launch_bounds__(ADAM_THREADS) void ema_guard_multi_kernel(const EmaArgs a, double ema_decay, const float *__restrict__ step,
                                                                       const pdgn_guard_record *__restrict__ guard) {
    if (guard->applied == 0.f) return;
    int lo = 0, hi = a.ntensors - 1;
    const int c = blockIdx.x;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.chunk0[mid] <= c) lo = mid; else hi = mid - 1;
    }
    float *const E = a.e[lo];
    const float *const P = a.p[lo];
    const long long n = a.n[lo], i0 = (long long)(c - a.chunk0[lo]) * ADAM_CHUNK;
    const float omd = ema_one_minus_decay(ema_decay, step);
    if (((((uintptr_t)E | (uintptr_t)P) & 15) == 0)) {
        constexpr int NU = ADAM_CHUNK / (4 * ADAM_THREADS);
        float4 e4[NU], p4[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const long long i = i0 + 4LL * (threadIdx.x + u * ADAM_THREADS);
            if (i + 3 < n) {
                e4[u] = *reinterpret_cast<const float4 *>(E + i);
                p4[u] = *reinterpret_cast<const float4 *>(P + i);
            }
        }
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const long long i = i0 + 4LL * (threadIdx.x + u * ADAM_THREADS);
            if (i + 3 < n) {
                ema_one(e4[u].x, p4[u].x, omd); ema_one(e4[u].y, p4[u].y, omd);
                ema_one(e4[u].z, p4[u].z, omd); ema_one(e4[u].w, p4[u].w, omd);
                *reinterpret_cast<float4 *>(E + i) = e4[u];
            } else {
                for (long long j = i; j < n && j < i + 4; ++j) ema_one(E[j], P[j], omd);
            }
        }
    } else {
        for (long long i = i0 + threadIdx.x; i < n && i < i0 + ADAM_CHUNK; i += ADAM_THREADS) ema_one(E[i], P[i], omd);
    }
}

__global__ __launch_bounds__(ADAM_THREADS) void ema_multi_kernel(const EmaArgs a, double ema_decay, const float *__restrict__ step) {
    int lo = 0, hi = a.ntensors - 1;
    const int c = blockIdx.x;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.chunk0[mid] <= c) lo = mid; else hi = mid - 1;
    }
    float *const E = a.e[lo];
    const float *const P = a.p[lo];
    const long long n = a.n[lo], i0 = (long long)(c - a.chunk0[lo]) * ADAM_CHUNK;
    const float omd = ema_one_minus_decay(ema_decay, step);
    if (((((uintptr_t)E | (uintptr_t)P) & 15) == 0)) {
        constexpr int NU = ADAM_CHUNK / (4 * ADAM_THREADS);
        float4 e4[NU], p4[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const long long i = i0 + 4LL * (threadIdx.x + u * ADAM_THREADS);
            if (i + 3 < n) {
                e4[u] = *reinterpret_cast<const float4 *>(E + i);
                p4[u] = *reinterpret_cast<const float4 *>(P + i);
            }
        }
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const long long i = i0 + 4LL * (threadIdx.x + u * ADAM_THREADS);
            if (i + 3 < n) {
                ema_one(e4[u].x, p4[u].x, omd); ema_one(e4[u].y, p4[u].y, omd);
                ema_one(e4[u].z, p4[u].z, omd); ema_one(e4[u].w, p4[u].w, omd);
                *reinterpret_cast<float4 *>(E + i) = e4[u];
            } else {
                for (long long j = i; j < n && j < i + 4; ++j) ema_one(E[j], P[j], omd);
            }
        }
    } else {
        for (long long i = i0 + threadIdx.x; i < n && i < i0 + ADAM_CHUNK; i += ADAM_THREADS) ema_one(E[i], P[i], omd);
    }
}

// e[i] (n[i] floats) <- e[i] + (1 - d_t) (p[i] - e[i]) for ntensors fp32 tensors (HOST arrays of device pointers, 4-byte aligned;
// 16-byte aligned pairs take the vector path), d_t = min(ema_decay, (1 + t) / (10 + t)) from step[0] (device), in
// ceil(ntensors / 128) launches.  No reference counterpart.
static int ema_multi_launch(int ntensors, void *const *e, const void *const *p, const long long *n, double ema_decay, const float *step,
                            const pdgn_guard_record *guard, pdgn_stream_t stream) {
    if (guard_misplaced(guard)) return PDGN_ERR_INVALID;
    if (ntensors < 1 || !e || !p || !n || !step || !(ema_decay >= 0. && ema_decay < 1.)) return PDGN_ERR_INVALID;
    for (int i = 0; i < ntensors; ++i)
        if (!e[i] || !p[i] || n[i] < 1 || (((uintptr_t)e[i] | (uintptr_t)p[i]) & 3)) return PDGN_ERR_INVALID;
    const int rc = for_each_launch<EmaArgs>(ntensors, n, [&](EmaArgs &a, int t0, unsigned chunks) {
        for (int i = 0; i < a.ntensors; ++i) { a.e[i] = (float *)e[t0 + i]; a.p[i] = (const float *)p[t0 + i]; }
        const dim3 grid(chunks), block(ADAM_THREADS);
        if (guard) hipLaunchKernelGGL(ema_guard_multi_kernel, grid, block, 0, (hipStream_t)stream, a, ema_decay, step, guard);
        else hipLaunchKernelGGL(ema_multi_kernel, grid, block, 0, (hipStream_t)stream, a, ema_decay, step);
    });
    return rc ? rc : pdgn_launch_status();
}

extern "C" int pdgn_ema_multi(int ntensors, void *const *e, const void *const *p, const long long *n, double ema_decay, const float *step,
                              pdgn_stream_t stream) {
    return ema_multi_launch(ntensors, e, p, n, ema_decay, step, nullptr, stream);
}

// pdgn_ema_multi behind a guarded optimizer step that was not pdgn_adam_ema_guard_multi: applied == 0 in the record leaves e as it is.
extern "C" int pdgn_ema_guard_multi(int ntensors, void *const *e, const void *const *p, const long long *n, double ema_decay,
                                    const float *step, const pdgn_guard_record *guard, pdgn_stream_t stream) {
    if (!guard) return PDGN_ERR_INVALID;
    return ema_multi_launch(ntensors, e, p, n, ema_decay, step, guard, stream);
}

static long long gradnorm_chunks(int ntensors, const long long *n) {
    if (ntensors < 1 || !n) return -1;
    for (int i = 0; i < ntensors; ++i)
        if (n[i] < 1) return -1;
    return list_chunks(ntensors, n, COPY_MAXT);
}

// Doubles of workspace pdgn_gradnorm_multi takes for this list: one per 4096-element chunk of every tensor; -1 for an invalid list.
extern "C" long long pdgn_gradnorm_workspace_doubles(int ntensors, const long long *n) { return gradnorm_chunks(ntensors, n); }

// The guard record of one network from its gradient list g (HOST array of device pointers, n: element counts): ceil(ntensors / 128)
// partial launches and one finalising launch on `stream`.  No reference counterpart (the reference applies every gradient unseen).
extern "C" int pdgn_gradnorm_multi(int ntensors, const void *const *g, const long long *n, double max_norm, double *workspace,
                                   long long workspace_doubles, pdgn_guard_record *record, pdgn_stream_t stream) {
    const long long total = gradnorm_chunks(ntensors, n);
    if (total < 1 || !g || !workspace || ((uintptr_t)workspace & 7) || workspace_doubles < total || !record || ((uintptr_t)record & 3) ||
        max_norm != max_norm)
        return PDGN_ERR_INVALID;
    for (int i = 0; i < ntensors; ++i)
        if (!g[i] || ((uintptr_t)g[i] & 3)) return PDGN_ERR_INVALID;
    long long done = 0;
    for_each_launch<GradArgs>(ntensors, n, [&](GradArgs &a, int t0, unsigned chunks) {
        for (int i = 0; i < a.ntensors; ++i) a.g[i] = (const float *)g[t0 + i];
        hipLaunchKernelGGL(gradnorm_partial_kernel, dim3(chunks), dim3(ADAM_THREADS), 0, (hipStream_t)stream, a, workspace + done);
        done += chunks;
    });
    hipLaunchKernelGGL(gradnorm_final_kernel, dim3(1), dim3(ADAM_THREADS), 0, (hipStream_t)stream, (const double *)workspace, total, max_norm,
                       record);
    return pdgn_launch_status();
}
