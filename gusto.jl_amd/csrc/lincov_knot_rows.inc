// lincov_knot_rows.inc -- the rows of knot k of lincov_kernel (lincov.hip), EVERY per-knot output: sigma_x, z_obs, Sxx (PLANT: Sxt;
// DENSE: the x-rows of S) from S_k in LDS, and sigma_u on the knots that have a control.  Included twice, as the live writer and
// as the loop that leaves zeros from a failed knot on: a new per-knot output is added here and is in both.  Text, not a lambda with a
// flag: every such lambda (flag at run or compile time, by-reference or by-value captures, the zero loop inside or outside)
// moved the register allocation of some instantiation past what it was (dubins PLANT DENSE: 14 -> 17 spilled SGPRs, or 142 ->
// 144 VGPRs; profiles/post_rollout.txt); as text the kernels' instruction bytes are those they had.
// In scope at the include: the kernel's constants and pointers, and
//   int k; bool with_u; double zk   the knot (1-based), whether it has a control, its z_obs
//   KNOT_ROWS_LIVE                  true: the values; false: zeros in their place.  Undefined again at the end of this text
if (lane < n) sx[(size_t)(k - 1) * n + lane] = KNOT_ROWS_LIVE ? sigma_of(sS[lane * NZ + lane]) : 0.0;
if (with_u && lane < m) su[(size_t)(k - 1) * m + lane] = KNOT_ROWS_LIVE ? sSu[lane] : 0.0;
if (lane == 0) zo[k - 1] = KNOT_ROWS_LIVE ? zk : 0.0;
if (Sall)
#pragma unroll
    for (int r = 0; r < RPF; r++) { const int e = lane + 64 * r; if (e < NPF) Sall[(size_t)(k - 1) * NPF + e] = KNOT_ROWS_LIVE ? sS[(e / n) * NZ + e % n] : 0.0; }
if constexpr (PLANT)
    if (Tall)
#pragma unroll
        for (int r = 0; r < RC; r++) { const int e = lane + 64 * r; if (e < NC) Tall[(size_t)(k - 1) * NC + e] = KNOT_ROWS_LIVE ? sS[(e / NT) * NZ + nz + e % NT] : 0.0; }
if constexpr (DENSE)
#pragma unroll
    for (int r = 0; r < RGZ; r++) { const int e = lane + 64 * r; if (e < NGZ) Rall[(size_t)(k - 1) * NGZ + e] = KNOT_ROWS_LIVE ? sS[e] : 0.0; }
#undef KNOT_ROWS_LIVE
