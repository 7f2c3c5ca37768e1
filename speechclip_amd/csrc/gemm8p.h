// Internal interface between gemm.hip (the sc_gemm_bf16 dispatcher) and gemm8p.hip (the ping-pong kernel).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"

struct Gemm8pParams {
    const bf16_t* A; int64_t lda;
    const bf16_t* W; int64_t ldw;
    void* C; int64_t ldc;              // bf16 / f16, or f32 when out_f32
    const float* bias;                 // may be null
    const void* residual; int64_t ldr;   // same element type as C
    int out_f32;
    int f16;                           // A, W (and C / residual unless out_f32) are IEEE half instead of bf16 (SC_GEMM_F16)
    int64_t M; int N; int K;
    int act;                           // SC_ACT_*
    int nk;                            // K / 64
    int tn;                            // N / 256
    int band;                          // N tiles per column band of the tile order (0: all of N)
    int sched;                         // in: >= 0 dynamic tile order allowed, -1 static; gemm8p.hip replaces it by the launch's counter slot
    unsigned sched_gen;                // set by gemm8p.hip: the launch's generation of that slot (see g_sched)
    unsigned long long* trace;         // PROBES: per-block cycle stamps
};

// gemm8p.hip.  0: launched; 1: shape outside the kernel's rules (nothing launched; the caller runs gemm256_kernel / gemm_bf16_kernel); < 0: error
int sc_gemm8p_try(const Gemm8pParams& p, hipStream_t s);

// gemm.hip.  Compute units of the current device, asked for once per process: the grid of every persistent GEMM kernel is one block per CU.
int sc_gemm_num_cus();
