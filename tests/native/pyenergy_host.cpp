// A generated Python-energy plugin source (ME_PYENERGY_SOURCE, a term dictionary) compiled for the host against the stub
// metropolis_user_energy.h next to this file, with C entry points for ctypes (tests/test_pyenergy_corpus_cpu.py).
#include ME_PYENERGY_SOURCE

template <typename R>
static void terms(int n, int d, const R *x, R *out) {
  for (int i = 0; i < n; ++i)
    for (int t = 0; t < ME_USER_N_TERMS; ++t)
      out[(long)i * ME_USER_N_TERMS + t] = me_user_energy_term<R>(t, x + (long)i * d, nullptr);
}

extern "C" int me_host_n_terms() { return ME_USER_N_TERMS; }
extern "C" unsigned me_host_term_groups(int term) { return me_user_term_groups(term); }
extern "C" void me_host_terms_f64(int n, int d, const double *x, double *out) { terms(n, d, x, out); }
extern "C" void me_host_terms_f32(int n, int d, const float *x, float *out) { terms(n, d, x, out); }

extern "C" int me_host_reject_f64(int n, int d, const double *x, unsigned char *out) {
#ifdef ME_USER_HAS_REJECT
  for (int i = 0; i < n; ++i) out[i] = me_user_reject<double>(x + (long)i * d, nullptr);
  return 1;
#else
  (void)n; (void)d; (void)x; (void)out;
  return 0;
#endif
}
