// Test infrastructure, not part of the library: the serial (host) forms of pcl_amd/csrc/ndt_forms.hpp behind a C ABI, so
// that tests/test_ndt_serial_forms.py can put nf::mt_trial_value, nf::mt_update_interval and nf::svd_solve6 beside their
// numpy restatement on states that no alignment of the suite reaches.  Built by that test with the flags of the wavefront
// emulation (tests/wavesim/Makefile: host clang++, -ffp-contract=off); the product library gains no export for it.
#include "ndt_forms.hpp"

using namespace pclhip;

extern "C" {

// I: a_l f_l g_l a_u f_u g_u
__attribute__((visibility("default"))) double ndt_test_trial_value(const double I[6], double a_t, double f_t, double g_t) {
  const nf::MtInterval S{I[0], I[1], I[2], I[3], I[4], I[5]};
  return nf::mt_trial_value(S, a_t, f_t, g_t);
}

__attribute__((visibility("default"))) int ndt_test_update_interval(double I[6], double a_t, double f_t, double g_t) {
  nf::MtInterval S{I[0], I[1], I[2], I[3], I[4], I[5]};
  const bool converged = nf::mt_update_interval(S, a_t, f_t, g_t);
  I[0] = S.a_l;
  I[1] = S.f_l;
  I[2] = S.g_l;
  I[3] = S.a_u;
  I[4] = S.f_u;
  I[5] = S.g_u;
  return converged ? 1 : 0;
}

__attribute__((visibility("default"))) void ndt_test_svd_solve6(const double H[36], const double b[6], double delta[6]) {
  nf::svd_solve6(H, b, delta);
}

}  // extern "C"
