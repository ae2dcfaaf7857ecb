// ab_stub_fixed_dt.cpp - lets a library built from a commit BEFORE the fixed-interval entries serve as the `--ab-lib` of
// tools/bench_fixed_dt.py: lcp_physics_amd/_lib.py binds every symbol include/lcp_hip.h declares when it loads a library, so the
// older build is linked together with these refusing stubs (the A/B workload, tools/bench_world.py, never calls them):
//
//   git archive PARENT lcp_physics_amd/csrc include tools/isa_lint.py | tar -x -C /tmp/parent && make -C /tmp/parent/lcp_physics_amd/csrc
//   hipcc -fPIC -c tools/ab_stub_fixed_dt.cpp -o /tmp/parent/stub.o
//   hipcc -shared -fPIC --offload-arch=gfx950 -o liblcp_parent.so /tmp/parent/lcp_physics_amd/csrc/*.o /tmp/parent/stub.o
extern "C" {
int lcp_move_find_contacts_dts_f64(...) { return -1; }   // LCP_E_BADARG
int lcp_substep_begin_f64(...) { return -1; }
int lcp_substep_commit_f32(...) { return -1; }
}
