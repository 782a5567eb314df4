// disparity_fill_mirror_test.cpp — SceneFlowConstructor::setDisparityFill exists and forwards to mod_set_disparity_fill, without the
// library: mirror_calls_test.cpp's call recorder stands in for it (its ModContext, its stubs and its Rig; its main is renamed and not
// run), and the one stub it lacks is defined here.  tests/test_disparity_fill_abi.py reads the lines that begin with the call's name.
#define main mirror_calls_main
#include "mirror_calls_test.cpp"
#undef main

int mod_set_disparity_fill(ModContext *c, const ModDisparityFill *f) {
  static_assert(sizeof(ModDisparityFill) == 16, "ModDisparityFill is 16 bytes");
  if (f) std::printf("mod_set_disparity_fill %d %d %d %d\n", f->reach, f->directions, f->mode, f->min_found);
  else std::printf("mod_set_disparity_fill NULL\n");
  return c->code("mod_set_disparity_fill");
}

int main() {
  Rig r;
  r.sfc.setDisparityFill(64, 8, MOD_DISPARITY_FILL_MIN, 1);
  r.sfc.setDisparityFill(256, 4, MOD_DISPARITY_FILL_MEDIAN, 3);
  r.sfc.setDisparityFill(0, 0, 0, 0);
  r.ctx.codes["mod_set_disparity_fill"] = {MOD_ERR_INVALID_ARGUMENT};     // a refusal becomes an exception, like every setter's
  try {
    r.sfc.setDisparityFill(16, 3, MOD_DISPARITY_FILL_SECOND, 1);
    std::printf("refused: returned\n");
  } catch (const std::runtime_error &) {
    std::printf("refused: threw\n");
  }
  return 0;
}
