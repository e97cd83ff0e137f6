// The body of k_w4_gemm64h (kernels_w4_f16.hip has its description), included as TEXT into k_w4_gemm64h and into the GEMM half of
// k_w4_gemm64h_wgrad64h (kernels_w4_wgrad.hip).  In scope where it is included: D (compile-time, the ring's depth), the kernel's
// parameters Vh, Uh, M, ctrl, gm, mode, v_exp, u_exp, stamps, and W4_BLOCK, the workgroup's index in the GEMM's own grid.
// Text and not a device function: w4s_pass_body.inc has the reason.
  if (ctrl != nullptr && ctrl->done) return;   // a step enqueued past the end of the interval (Ctrl::done)
  extern __shared__ __attribute__((aligned(16))) float smem[];   // [4 waves][2 blocks][4 r4][64 lanes][4]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned long long* st = stamps != nullptr ? stamps + ((size_t)W4_BLOCK * 4 + wave) * 16 : nullptr;   // (diagnostics build only)
  w4_stamp(st, 0);
  const int l31 = lane & 31, hi = lane >> 5;
  const int nCT = gm.C >> 6, nRB = gm.RB, G2 = gm.G8 >> 1, CB = gm.C >> 5;
  const int j = W4_BLOCK & 7, tile = W4_BLOCK >> 3;
  const int rt = tile / nCT, ct = tile - rt * nCT;
  const float inv = ldexpf(1.f, -(*v_exp + *u_exp));
  const int a_off = ((l31 >> 2) * 8) + hi * 4 + (l31 & 3);   // lane (row = 4 s + t, k-half hi): its 16 B inside a 1 KB part
  auto vblk = [&](int comp, int rb) { return reinterpret_cast<const w4_u32x4*>(Vh) + (((size_t)comp * nRB + rb) * G2) * 128 + a_off; };
  auto ublk = [&](int comp, int cb) { return reinterpret_cast<const w4_u32x4*>(Uh) + (((size_t)comp * CB + cb) * G2) * 128 + lane; };

  // the shared component's operands are requested behind the own component's first ring (one wave per SIMD: nothing else would
  // cover their latency at the end), and multiplied while the own component's stores drain
  constexpr int SH = 4;
  const int sng = G2 >> 2;                 // its K steps per wave
  const bool early = sng == SH;
  W4HStage shr[SH];
  const int scomp = 32 + (j >> 1), srb = 2 * rt + (j & 1);
  W4HCursor scu;
  scu.a[0] = vblk(scomp, srb) + (size_t)(wave * sng) * 128; scu.a[1] = scu.a[0];
  scu.b[0] = ublk(scomp, 2 * ct) + (size_t)(wave * sng) * 128; scu.b[1] = ublk(scomp, 2 * ct + 1) + (size_t)(wave * sng) * 128;
  {
    // mode bit 1 (NODE_TUNE_W4_SHAREV = 1, four column tiles): the four waves of a workgroup take the SAME component and row tile
    // and one column tile each (they walk the same V blocks in lock-step); bit 2: a 128 x 128 tile of one component (k_w4_gemm64b)
    const bool sharev = (mode & 2) != 0 && nCT == 4;
    const bool share2 = (mode & 4) != 0 && nCT == 4 && (nRB & 3) == 0;
    const int comp = 4 * j + (share2 ? (tile & 3) : sharev ? ct : wave);
    const int oct = share2 ? 2 * ((tile >> 2) & 1) + (wave & 1) : sharev ? wave : ct;
    const int ort = share2 ? 2 * (tile >> 3) + (wave >> 1) : rt;
    W4HCursor cu;
    cu.a[0] = vblk(comp, 2 * ort); cu.a[1] = vblk(comp, 2 * ort + 1);
    cu.b[0] = ublk(comp, 2 * oct); cu.b[1] = ublk(comp, 2 * oct + 1);
    float16_t acc[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[r][c][q] = 0.f;
    auto request_shared = [&]() {
      if (early) {
        W4HCursor c2 = scu;
#pragma unroll
        for (int i = 0; i < SH; ++i) {
          w4h_next<1>(shr[i], c2);
          __builtin_amdgcn_sched_barrier(0);
        }
        asm volatile("" ::: "memory");   // (the compiler may not sink these requests to their first use behind the loop)
      }
    };
    const size_t sstride = (size_t)(gm.C >> 5) * 36 * 128;   // floats per sample of M
    float* m0 = M + ((size_t)(ort * 16 + hi) * (gm.C >> 5) + 2 * oct) * (36 * 128) + (size_t)comp * 128 + l31;
    if ((mode & 16) != 0 && G2 % D == 0 && G2 >= 2 * D) {
      // mode bit 4 (no launcher sets it): the tile as TWO 32-row halves one after the other on ONE operand ring -- the first
      // half's 16 KB of results drain while the second half's operands stream in (as one 64 x 64 tile every wave of the chip loads, then
      // every wave stores: 3 us of a 12 us launch in which nothing is read); the column operand is fetched twice (from L2).
      W4HStage ring[D];
      W4HCursor cc;
      cc.a[0] = cu.a[0]; cc.a[1] = cu.a[0]; cc.b[0] = cu.b[0]; cc.b[1] = cu.b[1];
#pragma unroll
      for (int i = 0; i < D; ++i) {
        w4h_next<1>(ring[i], cc);
        __builtin_amdgcn_sched_barrier(0);
      }
      request_shared();
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        for (int g = 0; g < G2; g += D) {
          if (h == 0 && g + D == G2) { cc.a[0] = cu.a[1]; cc.b[0] = cu.b[0]; cc.b[1] = cu.b[1]; }   // this round's refills open the second half
#pragma unroll
          for (int i = 0; i < D; ++i) {
            w4h_mac<1>(acc, ring[i]);
            __builtin_amdgcn_sched_barrier(0);   // the refill stays behind the MFMAs that read the old contents
            w4h_next<1>(ring[i], cc);
          }
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          float* o = m0 + (size_t)(2 * (q >> 2)) * sstride + (q & 3) * 32 + (h ? 8 * sstride : 0);
          st_wt(o, acc[0][0][q] * inv);
          st_wt(o + 36 * 128, acc[0][1][q] * inv);
          acc[0][0][q] = 0.f; acc[0][1][q] = 0.f;
        }
      }
    } else {
      w4h_run<D, 2>(acc, cu, G2, request_shared, st);
      w4_stamp(st, 3);
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        float* o = m0 + (size_t)(2 * (q >> 2)) * sstride + (q & 3) * 32;
        st_wt(o, acc[0][0][q] * inv);
        st_wt(o + 36 * 128, acc[0][1][q] * inv);
        st_wt(o + 8 * sstride, acc[1][0][q] * inv);
        st_wt(o + 8 * sstride + 36 * 128, acc[1][1][q] * inv);
      }
      w4_stamp(st, 4);
    }
  }
  // --- half a tile of a shared component: rows [32 half, 32 half + 32), K range [wave G2/4, (wave+1) G2/4) per wave
  {
    float16_t acc[2][2];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[0][c][q] = 0.f;
    if (early) {
#pragma unroll
      for (int i = 0; i < SH; ++i) w4h_mac<1>(acc, shr[i]);
    } else if (sng % 4 == 0) w4h_run<4, 1>(acc, scu, sng);
    else if (sng % 2 == 0) w4h_run<2, 1>(acc, scu, sng);
    else w4h_run<1, 1>(acc, scu, sng);
    w4_stamp(st, 5);
    float* red = smem + wave * 2048;
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4)
        *reinterpret_cast<float4*>(red + c * 1024 + (r4 * 64 + lane) * 4) =
            make_float4(acc[0][c][4 * r4], acc[0][c][4 * r4 + 1], acc[0][c][4 * r4 + 2], acc[0][c][4 * r4 + 3]);
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int u = tid + it * 256;
      const int blk = u >> 8, r4 = (u >> 6) & 3;
      float4 sm = *reinterpret_cast<const float4*>(smem + blk * 1024 + (r4 * 64 + lane) * 4);
#pragma unroll
      for (int w = 1; w < 4; ++w) {
        const float4 v = *reinterpret_cast<const float4*>(smem + w * 2048 + blk * 1024 + (r4 * 64 + lane) * 4);
        sm.x += v.x; sm.y += v.y; sm.z += v.z; sm.w += v.w;
      }
      float* mrow = M + ((size_t)(srb * 8 + 2 * r4 + hi) * (gm.C >> 5) + 2 * ct + blk) * (36 * 128) + (size_t)scomp * 128 + l31;
      st_wt(mrow, sm.x * inv);
      st_wt(mrow + 32, sm.y * inv);
      st_wt(mrow + 64, sm.z * inv);
      st_wt(mrow + 96, sm.w * inv);
    }
  }
#ifdef NODE_DIAG
  if (st != nullptr) {   // (diagnostics: when this wave's stores have drained)
    w4_stamp(st, 6);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    w4_stamp(st, 7);
  }
#endif
