// The end of a sweep step (gfv/sweep.py: a trained model run over a device pool, slot by slot) as ONE launch - the sibling of
// rollout_advance_kernel (csrc/rollout.hip) with per-slot state on the device, so that one recorded launch replays for every step
// of every batch of a size signature:
//   live slot b (slots[b].done == 0 when the launch starts):
//     x_backup[:, 0:3] = uvp_node;  x = x_backup;  state3 = uvp_node          over the nodes of graph b
//     age += 1;  rel = || uvp_new - uvp_prev ||_2 / || uvp_new ||_2;  streak = rel < tol ? streak + 1 : 0
//     done = streak >= patience && age >= min_steps ? 1 : age >= max_steps ? 2 : 0
//     last[b] = (losses[b, 0:4], || uvp_new - uvp_prev ||_2, || uvp_new ||_2)
//   frozen slot (done != 0):  x = x_backup (x_backup is NOT overwritten);  state3 = x_backup[:, 0:3];  nothing else changes.
// `done` is read by phase 1 as the launch finds it and written by the workgroup that arrives last, after every workgroup has
// finished phase 1: the field a slot ends with is the prediction of the step that latched it, whatever is queued behind it.
// Summation order: csrc/gfv_reduce.h (the arrival counter is state[1], left at zero; all-fence form).
// With Anderson acceleration per slot (gfv_sweep_advance_aa, AA = true) the update just applied may be the mixed one: rel is
// formed from the true fixed-point residual || G(x) - x || / || G(x) || that gfv_sweep_anderson_gram left in aa_slot[b], and those
// two norms go to last[b, 4:6]; the update's own sums are not folded.  Everything else is the same instructions.
#include "../../include/gfv.h"
#include "gfv_common.h"
#include "gfv_launch.h"
#include "gfv_prof.h"
#include "gfv_reduce.h"

namespace {

constexpr int SW_WAVES = 4;

struct SweepCtl {
  float tol;                  // negative: never converge
  int min_steps, max_steps, patience;
};

struct SweepArgs {
  const float* uvp_node;      // [N,3]
  float* x_backup;            // [N,12]
  float* x;                   // [N,12]
  const int* chunk_beg;       // [n_chunks]
  const int* chunk_end;
  const int* gchunk_ptr;      // [B+1]
  const float* losses;        // [B,4]
  double* partial;            // [n_chunks,2]
  const SweepCtl* ctl;
  int* slots;                 // [B,4]: age, streak, done, reserved
  float* last;                // [B,6]
  float* state3;              // [N,3]
  int* mirror;                // pinned, device-mapped: [0] step sequence number, [1 + 2b] done, [2 + 2b] age
  int* state;                 // [2]: step sequence number, arrival counter
  const float* aa_slot;       // AA form: [B,4] (|| f ||, || g ||, depth, flags) of this step, per slot
  int N, n_chunks, B;
};

template <bool AA>
__global__ __launch_bounds__(64 * SW_WAVES) void sweep_advance_kernel(const SweepArgs A) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = blockIdx.x * SW_WAVES + wave;
  if (c < A.n_chunks) {
    const int b = gfv_chunk_graph(A.gchunk_ptr, A.B, c);
    const bool live = A.slots[4 * b + 2] == 0;
    const int beg = A.chunk_beg[c], end = min(A.chunk_end[c], A.N);
    double d2 = 0.0, n2 = 0.0;
    for (int i = beg + lane; i < end; i += 64) {
      if (i < 0) continue;
      const float4 r0 = gfv_advance_row(A.uvp_node, A.x_backup, A.x, i, live, d2, n2);
      float* s3 = A.state3 + (size_t)i * 3;
      s3[0] = r0.x; s3[1] = r0.y; s3[2] = r0.z;
    }
    if (!AA) {
      d2 = gfv_wave_sum(d2);
      n2 = gfv_wave_sum(n2);
      if (lane == 0) {
        A.partial[2 * (size_t)c] = d2;
        A.partial[2 * (size_t)c + 1] = n2;
      }
    }
  }
  if (!gfv_arrive_last_all_fence(A.state + 1)) return;
  const float tol = A.ctl->tol;
  const int min_steps = A.ctl->min_steps, max_steps = A.ctl->max_steps, patience = A.ctl->patience;
  for (int b = wave; b < A.B; b += SW_WAVES) {
    int* s = A.slots + 4 * b;
    int age = s[0], streak = s[1], done = s[2];
    if (done == 0) {
      float dn, un;
      if (AA) {
        dn = A.aa_slot[4 * (size_t)b];
        un = A.aa_slot[4 * (size_t)b + 1];
      } else {
        const int c0 = A.gchunk_ptr[b], c1 = min(A.gchunk_ptr[b + 1], A.n_chunks);
        double p[2];
        gfv_fold_chunks(A.partial, c0, c1, lane, p);
        const double d2 = gfv_wave_sum(p[0]), n2 = gfv_wave_sum(p[1]);
        dn = (float)sqrt(d2);
        un = (float)sqrt(n2);
      }
      const float rel = dn / un;                 // (0 / 0 and x / 0: NaN and inf compare false)
      age += 1;
      streak = rel < tol ? streak + 1 : 0;
      if (streak >= patience && age >= min_steps) done = 1;
      else if (age >= max_steps) done = 2;
      float* h = A.last + 6 * (size_t)b;
      if (lane < 4) h[lane] = A.losses[4 * b + lane];
      if (lane == 4) h[4] = dn;
      if (lane == 5) h[5] = un;
      if (lane == 0) { s[0] = age; s[1] = streak; s[2] = done; }
    }
    if (lane == 0) {
      __hip_atomic_store(A.mirror + 1 + 2 * b, done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(A.mirror + 2 + 2 * b, age, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  __threadfence_system();
  __syncthreads();
  // (per-lane vector stores of the two counters)
  if (tid == 0) {
    const int seq = A.state[0] + 1;
    A.state[0] = seq;
    A.state[1] = 0;
    __hip_atomic_store(A.mirror, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

}  // namespace

extern "C" int gfv_sweep_mirror_create(int32_t n_words, int32_t** host_words, int32_t** dev_words) {
  if (n_words <= 0 || !host_words || !dev_words) return GFV_ERR_ARG;
  void* h = nullptr;
  void* d = nullptr;
  if (hipHostMalloc(&h, sizeof(int32_t) * (size_t)n_words, hipHostMallocMapped) != hipSuccess) return GFV_ERR_LAUNCH;
  for (int32_t i = 0; i < n_words; ++i) static_cast<int32_t*>(h)[i] = 0;
  if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
    (void)hipHostFree(h);
    return GFV_ERR_LAUNCH;
  }
  *host_words = static_cast<int32_t*>(h);
  *dev_words = static_cast<int32_t*>(d);
  return GFV_OK;
}

extern "C" int gfv_sweep_mirror_free(int32_t* host_words) {
  if (!host_words) return GFV_ERR_ARG;
  return hipHostFree(host_words) == hipSuccess ? GFV_OK : GFV_ERR_LAUNCH;
}

namespace {

int sweep_advance_launch(const float* uvp_node, float* x_backup, float* x, int32_t N, const int32_t* chunk_beg,
                         const int32_t* chunk_end, const int32_t* gchunk_ptr, int32_t n_chunks, int32_t B, const float* losses,
                         double* partial_ws, const void* ctl, int32_t* slots, float* last, float* state3, int32_t* mirror_dev,
                         int32_t* state, const float* aa_slot, bool aa, void* stream) {
  if (!uvp_node || !x_backup || !x || !chunk_beg || !chunk_end || !gchunk_ptr || !losses || !partial_ws || !ctl || !slots ||
      !last || !state3 || !mirror_dev || !state || (aa && !aa_slot))
    return GFV_ERR_ARG;
  if (N <= 0 || n_chunks <= 0 || B <= 0) return GFV_ERR_ARG;
  if ((reinterpret_cast<size_t>(x_backup) | reinterpret_cast<size_t>(x)) & 15) return GFV_ERR_ARG;
  // rows: uvp [N,3] read, x_backup [N,12] read, 16 B of it, x [N,12] and state3 [N,3] written
  GfvProfScope ps_(GFV_K_MISC, 0, (12.0 + 48.0 + 16.0 + 48.0 + 12.0) * N, stream);
  const SweepArgs a{uvp_node, x_backup, x, chunk_beg, chunk_end, gchunk_ptr, losses, partial_ws,
                    static_cast<const SweepCtl*>(ctl), slots, last, state3, mirror_dev, state, aa_slot, N, n_chunks, B};
  const dim3 grid((n_chunks + SW_WAVES - 1) / SW_WAVES), block(64 * SW_WAVES);
  if (aa) GFV_LAUNCH(sweep_advance_kernel<true>, grid, block, 0, (hipStream_t)stream, a);
  else GFV_LAUNCH(sweep_advance_kernel<false>, grid, block, 0, (hipStream_t)stream, a);
  GFV_CHECK_LAUNCH();
  return GFV_OK;
}

}  // namespace

extern "C" int gfv_sweep_advance(const float* uvp_node, float* x_backup, float* x, int32_t N, const int32_t* chunk_beg,
                                 const int32_t* chunk_end, const int32_t* gchunk_ptr, int32_t n_chunks, int32_t B,
                                 const float* losses, double* partial_ws, const void* ctl, int32_t* slots, float* last,
                                 float* state3, int32_t* mirror_dev, int32_t* state, void* stream) {
  return sweep_advance_launch(uvp_node, x_backup, x, N, chunk_beg, chunk_end, gchunk_ptr, n_chunks, B, losses, partial_ws, ctl,
                              slots, last, state3, mirror_dev, state, nullptr, false, stream);
}

extern "C" int gfv_sweep_advance_aa(const float* uvp_node, float* x_backup, float* x, int32_t N, const int32_t* chunk_beg,
                                    const int32_t* chunk_end, const int32_t* gchunk_ptr, int32_t n_chunks, int32_t B,
                                    const float* losses, double* partial_ws, const void* ctl, int32_t* slots, float* last,
                                    float* state3, int32_t* mirror_dev, int32_t* state, const float* aa_slot, void* stream) {
  return sweep_advance_launch(uvp_node, x_backup, x, N, chunk_beg, chunk_end, gchunk_ptr, n_chunks, B, losses, partial_ws, ctl,
                              slots, last, state3, mirror_dev, state, aa_slot, true, stream);
}
