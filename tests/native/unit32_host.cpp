/* Num<float>::unit (metropolisengine_amd/csrc/me_device.h) restated for the host, for tests/test_draw_reference_cpu.py:
   the word as a float32, then ONE fused multiply-add.  Build without -ffast-math. */
#include <math.h>
#include <stdint.h>

extern "C" void me_unit_f32(const uint32_t *w, long n, float *out) {
  for (long i = 0; i < n; ++i) out[i] = fmaf((float)w[i], 2.3283064365386963e-10f, 1.1641532182693481e-10f);
}
