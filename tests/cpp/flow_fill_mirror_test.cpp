// flow_fill_mirror_test.cpp — SceneFlowConstructor::setFlowFill exists and forwards to mod_set_flow_fill, without the library:
// mirror_calls_test.cpp's call recorder stands in for it (its ModContext, its stubs and its Rig; its main is renamed and not run), and
// the one stub it lacks is defined here.  tests/test_flow_fill_abi.py reads the lines that begin with the call's name.
#define main mirror_calls_main
#include "mirror_calls_test.cpp"
#undef main

int mod_set_flow_fill(ModContext *c, const ModFlowFill *f) {
  static_assert(sizeof(ModFlowFill) == 24, "ModFlowFill is 24 bytes");
  if (f) std::printf("mod_set_flow_fill %d %d %g %g %d %d\n", f->window, f->min_valid, f->tol_abs, f->tol_rel, f->reserved[0], f->reserved[1]);
  else std::printf("mod_set_flow_fill NULL\n");
  return c->code("mod_set_flow_fill");
}

int main() {
  Rig r;
  r.sfc.setFlowFill(5, 3, 1.0f, 0.0f);
  r.sfc.setFlowFill(7, 48, 0.25f, 0.0625f);
  r.sfc.setFlowFill(0, 0, 0.0f, 0.0f);
  r.ctx.codes["mod_set_flow_fill"] = {MOD_ERR_INVALID_ARGUMENT};     // a refusal becomes an exception, like every setter's
  try {
    r.sfc.setFlowFill(4, 1, 1.0f, 0.0f);
    std::printf("refused: returned\n");
  } catch (const std::runtime_error &) {
    std::printf("refused: threw\n");
  }
  return 0;
}
