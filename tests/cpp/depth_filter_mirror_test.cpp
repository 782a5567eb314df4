// depth_filter_mirror_test.cpp — SceneFlowConstructor::setDepthFilter exists and forwards to mod_set_depth_filter, without the
// library: mirror_calls_test.cpp's call recorder stands in for it (its ModContext, its stubs and its Rig; its main is renamed and not
// run), and the one stub it lacks is defined here.  tests/test_depth_filter_abi.py reads the lines that begin with the call's name.
#define main mirror_calls_main
#include "mirror_calls_test.cpp"
#undef main

int mod_set_depth_filter(ModContext *c, const ModDepthFilter *f) {
  if (f) std::printf("mod_set_depth_filter %g %g %d %d %g %g %d %d\n", f->z_min, f->z_max, f->window, f->min_support, f->tol_abs, f->tol_rel, f->reserved[0], f->reserved[1]);
  else std::printf("mod_set_depth_filter NULL\n");
  return c->code("mod_set_depth_filter");
}

int main() {
  Rig r;
  const ModDepthFilter f{0.5f, 6.0f, 5, 7, 0.01f, 0.03f, {0, 0}};
  r.sfc.setDepthFilter(&f);
  r.sfc.setDepthFilter(nullptr);
  r.ctx.codes["mod_set_depth_filter"] = {MOD_ERR_INVALID_ARGUMENT};     // a refusal becomes an exception, like every setter's
  try {
    r.sfc.setDepthFilter(&f);
    std::printf("refused: returned\n");
  } catch (const std::runtime_error &) {
    std::printf("refused: threw\n");
  }
  return 0;
}
