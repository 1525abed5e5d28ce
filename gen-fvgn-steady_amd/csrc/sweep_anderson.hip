// Anderson acceleration AA(m) per slot of a sweep (gfv/sweep.py, gfv/anderson.py SlotAndersonState): the SLOT
// form's two entry points - two launches between the forward-only step and gfv_sweep_advance_aa (csrc/sweep.hip), decided on the
// device so that one recorded launch list per batch signature serves the whole sweep.  The kernels, the algorithm and the
// summation order are in csrc/anderson_kernel.h, which the rollout form (csrc/anderson.hip) instantiates too; what the slot form
// adds - rings per slot, the slot's own age as the step index, frozen slots skipped, the below-tol rule, records per slot - is
// stated at the head of that file.
#include "../../include/gfv.h"
#include "anderson_kernel.h"
#include "gfv_common.h"
#include "gfv_launch.h"
#include "gfv_prof.h"

extern "C" int gfv_sweep_anderson_gram(const float* uvp_node, const float* x_backup, int32_t N, const int32_t* chunk_beg,
                                       const int32_t* chunk_end, const int32_t* gchunk_ptr, int32_t n_chunks, int32_t B, int32_t m,
                                       double reg, double restart, int32_t start, int32_t ring_stride, float* f_prev, float* g_prev,
                                       float* dF, float* dG, int32_t* aa_state, double* r_prev, double* gamma, double* partial_ws,
                                       int32_t* counter, const void* ctl, const int32_t* slots, float* aa_slot, int32_t* aa_count,
                                       void* stream) {
  if (!uvp_node || !x_backup || !f_prev || !g_prev || !dF || !dG || !aa_state || !r_prev || !gamma || !partial_ws || !counter ||
      !ctl || !slots || !aa_slot || !aa_count)
    return GFV_ERR_ARG;
  if (aa_bad_tables(chunk_beg, chunk_end, gchunk_ptr, N, n_chunks, B, m) || ring_stride <= 0) return GFV_ERR_ARG;
  if (aa_bad_gram_numbers(reg, restart)) return GFV_ERR_ARG;
  if (aa_misaligned8(r_prev, gamma, partial_ws)) return GFV_ERR_ARG;
  GfvProfScope ps_(GFV_K_MISC, 0, aa_gram_bytes(m) * N, stream);
  const GramArgs a{uvp_node, x_backup, chunk_beg, chunk_end, gchunk_ptr, f_prev, g_prev, dF, dG, aa_state, r_prev, gamma,
                   partial_ws, counter, nullptr, nullptr, static_cast<const float*>(ctl), slots, aa_slot, aa_count, reg, restart,
                   N, n_chunks, B, 0, m, start, ring_stride};
  GFV_LAUNCH(anderson_gram_kernel<true>, dim3((n_chunks + AA_WAVES - 1) / AA_WAVES), dim3(64 * AA_WAVES), 0, (hipStream_t)stream, a);
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}

extern "C" int gfv_sweep_anderson_mix(float* uvp_node, const float* f_cur, int32_t N, const int32_t* chunk_beg,
                                      const int32_t* chunk_end, const int32_t* gchunk_ptr, int32_t n_chunks, int32_t B, int32_t m,
                                      double beta, int32_t ring_stride, const float* dF, const float* dG, const double* gamma,
                                      const int32_t* slots, const float* aa_slot, void* stream) {
  if (!uvp_node || !f_cur || !dF || !dG || !gamma || !slots || !aa_slot) return GFV_ERR_ARG;
  if (aa_bad_tables(chunk_beg, chunk_end, gchunk_ptr, N, n_chunks, B, m) || ring_stride <= 0) return GFV_ERR_ARG;
  if (aa_bad_beta(beta)) return GFV_ERR_ARG;
  if (reinterpret_cast<size_t>(gamma) & 7) return GFV_ERR_ARG;
  GfvProfScope ps_(GFV_K_MISC, 0, aa_mix_bytes(m, beta) * N, stream);
  const MixArgs a{uvp_node, f_cur, chunk_beg, chunk_end, gchunk_ptr, dF, dG, gamma, nullptr, nullptr, slots, aa_slot, 1.0 - beta,
                  N, n_chunks, B, 0, m, ring_stride};
  GFV_LAUNCH(anderson_mix_kernel<true>, dim3((n_chunks + AA_WAVES - 1) / AA_WAVES), dim3(64 * AA_WAVES), 0, (hipStream_t)stream, a);
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}
