// post_transform.h -- the element transforms between a network posterior and the log-posterior a dynamic programme consumes:
// decode.prepare_post (sloika/decode.py:36), np.log(trans) (sloika/transducer.py:30) and log(post + eta) (decode.py:56).  One
// definition for every kernel that applies them (decode.hip, event_remap.hip), so that they give the same bits by construction.
#pragma once
#include "common.h"

#define VIT_ETA 1e-10f

// exact restatement of numpy's float32 evaluation; __fmul_rn/__fadd_rn stop hipcc fusing the pair into an fma
__device__ __forceinline__ float prepare_post_val(float p, float min_prob, float one_m)
{
    return __fadd_rn(min_prob, __fmul_rn(one_m, p));       // decode.py:36
}

// natural log through v_log_f32 (log2) * ln2: ~1e-7 relative, 2 instructions instead of ~20 -- the decoder evaluates
// it once per (t, chunk, state), i.e. 840 M times per B=1024 batch
__device__ __forceinline__ float fast_logf(float x) { return __builtin_amdgcn_logf(x) * 0.6931471805599453f; }

__device__ __forceinline__ float log_post_val(float p, int mode, float min_prob, float one_m)
{
    if (mode == SLK_POST_LOG) return p;
    if (mode == SLK_POST_LN) return fast_logf(p);          // transducer.py:30
    if (mode == SLK_POST_RAW) p = prepare_post_val(p, min_prob, one_m);
    return fast_logf(__fadd_rn(p, VIT_ETA));               // decode.py:56
}

// (1.0 - min_prob) is evaluated in double by the reference and THEN cast to float32 (decode.py:36)
static inline float one_minus(float min_prob_f, double min_prob_d) { (void)min_prob_f; return (float)(1.0 - min_prob_d); }
