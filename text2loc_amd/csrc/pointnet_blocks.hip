// Dev-only block library (libt2l_blocks.so; never shipped, not part of include/t2l.h): the eval-mode PointNet++ backbone stage by
// stage, so that tests/test_gpu_pointnet_blocks.py can hold every level against a float64 reference element by element.
// This translation unit IS pointnet.hip plus the wrappers below and is linked in pointnet.o's place: a context made through the
// blocks library runs the product's own launch path (t2l_pointnet_features), and the door below copies what that call left in the
// context's workspace (PointNetLevels). No kernel and no grid expression lives here.
//
// Return: 0, -1 (refused, message through t2l_blk_last_error; nothing was copied or launched), -2 (the HIP runtime reported an error).
#include "pointnet.hip"
#include "blocks_common.h"

using namespace t2l;

extern "C" {

// The level buffers of objects [first, first + count) of the LAST t2l_pointnet_features call of `ctx`, which served n_obj objects:
//   p1 [count][128][3]  x1 [count][128][64]   p2 [count][64][3]  x2 [count][64][128]   p3 [count][32][3]  x3 [count][32][256]
//   f0 [count][1024]    f1 [count][512]       flags int32[count]: the magnitude watch (all 0 after an encoder_f32 call: no watch ran)
// Device pointers; null = skip. The whole device is synchronised first (the call may still be running on its stream).
int t2l_blk_pointnet_levels(t2l_ctx* ctx, int n_obj, int first, int count, float* p1, float* x1, float* p2, float* x2, float* p3, float* x3,
                            float* f0, float* f1, int32_t* flags) {
  const std::string who = "t2l_blk_pointnet_levels";
  if (!ctx) return blk_refuse(who + ": null context");
  const PointNetWeights* W = reinterpret_cast<const PointNetWeights*>(ctx->pn);
  if (!W || !W->ws || W->last_n_obj <= 0) return blk_refuse(who + ": no t2l_pointnet_features call has completed on this context");
  if (n_obj != W->last_n_obj)
    return blk_refuse(who + ": n_obj = " + std::to_string(n_obj) + ", but the last call served " + std::to_string(W->last_n_obj) + " objects");
  if (PointNetLevels::bytes(n_obj) > W->ws_cap) return blk_refuse(who + ": the workspace is smaller than the last call's levels (internal error)");
  if (first < 0 || count < 1 || first > n_obj - count) return blk_refuse(who + ": need 0 <= first, 1 <= count, first + count <= n_obj");
  auto failed = [&](hipError_t e) {
    if (e != hipSuccess) blk_refuse(who + ": " + hipGetErrorString(e));
    return e != hipSuccess;
  };
  if (failed(hipSetDevice(ctx->device)) || failed(hipDeviceSynchronize())) return -2;
  const PointNetLevels L(W->ws, n_obj);
  const size_t lo = (size_t)first, n = (size_t)count;
  struct Part {
    void* dst;
    const void* src;
    size_t bytes;
  };
  const Part parts[] = {
      {p1, L.p1 + lo * 128 * 3, n * 128 * 3 * sizeof(float)},   {x1, L.x1 + lo * 128 * 64, n * 128 * 64 * sizeof(float)},
      {p2, L.p2 + lo * 64 * 3, n * 64 * 3 * sizeof(float)},     {x2, L.x2 + lo * 64 * 128, n * 64 * 128 * sizeof(float)},
      {p3, L.p3 + lo * 32 * 3, n * 32 * 3 * sizeof(float)},     {x3, L.x3 + lo * 32 * 256, n * 32 * 256 * sizeof(float)},
      {f0, L.f0 + lo * 1024, n * 1024 * sizeof(float)},         {f1, L.f1 + lo * 512, n * 512 * sizeof(float)},
  };
  for (const Part& p : parts)
    if (p.dst && failed(hipMemcpyAsync(p.dst, p.src, p.bytes, hipMemcpyDeviceToDevice, nullptr))) return -2;
  if (flags) {
    const hipError_t e = W->last_flags ? hipMemcpyAsync(flags, L.flags + lo, n * sizeof(int32_t), hipMemcpyDeviceToDevice, nullptr)
                                       : hipMemsetAsync(flags, 0, n * sizeof(int32_t), nullptr);
    if (failed(e)) return -2;
  }
  return blk_finish("t2l_blk_pointnet_levels");
}

// pn_fps_kernel<NS> alone: dst_pos [n_obj][NS / 2][3] = the centres of src_pos [n_obj][NS][3], NS 256, 128 or 64 (the three levels).
// flags (optional) int32[n_obj]: objects with a non-zero flag are skipped, as in the product's launch.
int t2l_blk_pn_fps(const float* src_pos, float* dst_pos, const int32_t* flags, int n_obj, int ns) {
  const std::string who = "t2l_blk_pn_fps";
  if (!src_pos || !dst_pos) return blk_refuse(who + ": null pointer");
  if (n_obj < 1 || n_obj > (1 << 20)) return blk_refuse(who + ": need 1 <= n_obj <= 2^20");
  const dim3 grid((n_obj + 3) / 4), block(256);
  if (ns == 256) hipLaunchKernelGGL((pn_fps_kernel<256>), grid, block, 0, nullptr, src_pos, dst_pos, flags, n_obj);
  else if (ns == 128) hipLaunchKernelGGL((pn_fps_kernel<128>), grid, block, 0, nullptr, src_pos, dst_pos, flags, n_obj);
  else if (ns == 64) hipLaunchKernelGGL((pn_fps_kernel<64>), grid, block, 0, nullptr, src_pos, dst_pos, flags, n_obj);
  else return blk_refuse(who + ": ns must be 256, 128 or 64 (the instances the backbone builds)");
  return blk_finish("t2l_blk_pn_fps");
}

}  // extern "C"
