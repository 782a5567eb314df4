// depth_spatial_mirror_test.cpp — SceneFlowConstructor::setDepthSpatial exists and forwards to mod_set_depth_spatial, without the
// library: mirror_calls_test.cpp's call recorder stands in for it (its ModContext, its stubs and its Rig; its main is renamed and not
// run), and the one stub it lacks is defined here.  tests/test_depth_spatial_abi.py reads the lines that begin with the call's name.
#define main mirror_calls_main
#include "mirror_calls_test.cpp"
#undef main

int mod_set_depth_spatial(ModContext *c, const ModDepthSpatial *s) {
  if (s) std::printf("mod_set_depth_spatial %d %d %d %g %g %d %d %d\n", s->window, s->smooth, s->fill_min, s->tol_abs, s->tol_rel, s->reserved[0], s->reserved[1], s->reserved[2]);
  else std::printf("mod_set_depth_spatial NULL\n");
  return c->code("mod_set_depth_spatial");
}

int main() {
  Rig r;
  const ModDepthSpatial s{5, 1, 6, 0.25f, 0.125f, {0, 0, 0}};
  r.sfc.setDepthSpatial(&s);
  r.sfc.setDepthSpatial(nullptr);
  r.ctx.codes["mod_set_depth_spatial"] = {MOD_ERR_INVALID_ARGUMENT};     // a refusal becomes an exception, like every setter's
  try {
    r.sfc.setDepthSpatial(&s);
    std::printf("refused: returned\n");
  } catch (const std::runtime_error &) {
    std::printf("refused: threw\n");
  }
  return 0;
}
