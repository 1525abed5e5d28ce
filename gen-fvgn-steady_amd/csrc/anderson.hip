// Anderson acceleration AA(m) of the steady-state rollout (gfv/rollout.py, gfv/anderson.py): TWO launches between the
// forward-only step and gfv_rollout_advance, decided on the device so that one recorded launch list serves every step.  This file
// is the ROLLOUT form's two entry points; the kernels, the algorithm and the summation order are in csrc/anderson_kernel.h, which
// the slot form (csrc/sweep_anderson.hip) instantiates too.
#include "../../include/gfv.h"
#include "anderson_kernel.h"
#include "gfv_common.h"
#include "gfv_launch.h"
#include "gfv_prof.h"

extern "C" int gfv_anderson_gram(const float* uvp_node, const float* x_backup, int32_t N, const int32_t* chunk_beg,
                                 const int32_t* chunk_end, const int32_t* gchunk_ptr, int32_t n_chunks, int32_t B, int32_t m,
                                 double reg, double restart, int32_t start, float* f_prev, float* g_prev, float* dF, float* dG,
                                 int32_t* aa_state, double* r_prev, double* gamma, double* partial_ws, int32_t* counter,
                                 float* aa_table, int32_t K_max, const int32_t* step, void* stream) {
  if (!uvp_node || !x_backup || !f_prev || !g_prev || !dF || !dG || !aa_state || !r_prev || !gamma || !partial_ws || !counter ||
      !aa_table || !step)
    return GFV_ERR_ARG;
  if (aa_bad_tables(chunk_beg, chunk_end, gchunk_ptr, N, n_chunks, B, m) || K_max <= 0) return GFV_ERR_ARG;
  if (aa_bad_gram_numbers(reg, restart)) return GFV_ERR_ARG;
  if (aa_misaligned8(r_prev, gamma, partial_ws)) return GFV_ERR_ARG;
  // rows: uvp [N,3] and 12 B of x_backup read, f_prev / g_prev read and written, one ring column of dF / dG written, up to m of
  // dF read
  GfvProfScope ps_(GFV_K_MISC, 0, aa_gram_bytes(m) * N, stream);
  const GramArgs a{uvp_node, x_backup, chunk_beg, chunk_end, gchunk_ptr, f_prev, g_prev, dF, dG, aa_state, r_prev, gamma,
                   partial_ws, counter, aa_table, step, nullptr, nullptr, nullptr, nullptr, reg, restart, N, n_chunks, B, K_max, m,
                   start, 0};
  GFV_LAUNCH(anderson_gram_kernel<false>, dim3((n_chunks + AA_WAVES - 1) / AA_WAVES), dim3(64 * AA_WAVES), 0, (hipStream_t)stream, a);
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}

extern "C" int gfv_anderson_mix(float* uvp_node, const float* f_cur, int32_t N, const int32_t* chunk_beg, const int32_t* chunk_end,
                                const int32_t* gchunk_ptr, int32_t n_chunks, int32_t B, int32_t m, double beta, const float* dF,
                                const float* dG, const double* gamma, const float* aa_table, int32_t K_max, const int32_t* step,
                                void* stream) {
  if (!uvp_node || !f_cur || !dF || !dG || !gamma || !aa_table || !step) return GFV_ERR_ARG;
  if (aa_bad_tables(chunk_beg, chunk_end, gchunk_ptr, N, n_chunks, B, m) || K_max <= 0) return GFV_ERR_ARG;
  if (aa_bad_beta(beta)) return GFV_ERR_ARG;
  if (reinterpret_cast<size_t>(gamma) & 7) return GFV_ERR_ARG;
  // rows of an accelerated graph: uvp read and written, up to m columns of dG (and, with beta < 1, f and dF) read
  GfvProfScope ps_(GFV_K_MISC, 0, aa_mix_bytes(m, beta) * N, stream);
  const MixArgs a{uvp_node, f_cur, chunk_beg, chunk_end, gchunk_ptr, dF, dG, gamma, aa_table, step, nullptr, nullptr, 1.0 - beta,
                  N, n_chunks, B, K_max, m, 0};
  GFV_LAUNCH(anderson_mix_kernel<false>, dim3((n_chunks + AA_WAVES - 1) / AA_WAVES), dim3(64 * AA_WAVES), 0, (hipStream_t)stream, a);
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}
