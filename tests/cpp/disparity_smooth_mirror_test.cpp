// disparity_smooth_mirror_test.cpp — SceneFlowConstructor::setDisparitySmooth exists and forwards to mod_set_disparity_smooth, without the
// library: mirror_calls_test.cpp's call recorder stands in for it (its ModContext, its stubs and its Rig; its main is renamed and not
// run), and the one stub it lacks is defined here.  tests/test_disparity_smooth_abi.py reads the lines that begin with the call's name.
#define main mirror_calls_main
#include "mirror_calls_test.cpp"
#undef main

int mod_set_disparity_smooth(ModContext *c, const ModDisparitySmooth *f) {
  static_assert(sizeof(ModDisparitySmooth) == 16, "ModDisparitySmooth is 16 bytes");
  if (f) std::printf("mod_set_disparity_smooth %d %d %g %d\n", f->window, f->min_members, (double)f->tol, f->reserved);
  else std::printf("mod_set_disparity_smooth NULL\n");
  return c->code("mod_set_disparity_smooth");
}

int main() {
  Rig r;
  r.sfc.setDisparitySmooth(5, 1.0f, 1);
  r.sfc.setDisparitySmooth(7, 0.0625f, 49);
  r.sfc.setDisparitySmooth(0, 0.0f, 0);      // off: NULL
  r.ctx.codes["mod_set_disparity_smooth"] = {MOD_ERR_INVALID_ARGUMENT};     // a refusal becomes an exception, like every setter's
  try {
    r.sfc.setDisparitySmooth(4, 1.0f, 1);
    std::printf("refused: returned\n");
  } catch (const std::runtime_error &) {
    std::printf("refused: threw\n");
  }
  return 0;
}
