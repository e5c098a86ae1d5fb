// Prints the plan vimo_clip_amd/csrc/attn_route.h gives to each call described on stdin, one per line, so that
// tests/test_attention_refs_host.py can hold the Python port in tests/attention_refs.py (which the attention parity tests use to
// assert the kernel family of every case) against the header itself.  Built with g++ by that test.
//   vit N NQ F H variant                                   -> kernel vit|nc grid
//   fwd B H Tq Tk dh ld out_off                            -> kernel
//   bwd B H Tq Tk dh ld lddq ldo grad_off out_off          -> kernel block rs
// Pointers are only tested by the route, never dereferenced: a fixed 4096-aligned address plus the byte offset stands in.
#include <cstdio>
#include <cstring>

#include "../../vimo_clip_amd/csrc/attn_route.h"

static const char* kname(const AttnPlan& p) {
  static const char* n[] = {"ATTN_VIT", "ATTN_VIT_LONG", "ATTN_VIT_LONG_CLS", "ATTN_SMALL", "ATTN_LONG_FWD", "ATTN_GENERIC_FWD",
                            "ATTN_BWD_MFMA", "ATTN_LONG_BWD", "ATTN_GENERIC_BWD"};
  return p.rc == VMC_E_SHAPE ? "E_SHAPE" : p.rc ? "ERR" : n[p.kernel];
}

int main() {
  char kind[16];
  char* const base = (char*)(uintptr_t)0x10000;
  while (scanf("%15s", kind) == 1) {
    if (!strcmp(kind, "vit")) {
      int N, NQ, F, H, variant;
      if (scanf("%d %d %d %d %d", &N, &NQ, &F, &H, &variant) != 5) return 2;
      AttnVitProblem p{base, base, base, base, nullptr, 0, 0, F, N, NQ, H, VMC_BF16};
      AttnOverrides ov;
      ov.variant = variant;
      const AttnPlan pl = attn_vit_route(p, ov);
      printf("%s %d %u\n", kname(pl), pl.kernel == ATTN_VIT ? pl.vit : pl.nc, pl.grid[0]);
    } else if (!strcmp(kind, "fwd")) {
      int B, H, Tq, Tk, dh, ld, off;
      if (scanf("%d %d %d %d %d %d %d", &B, &H, &Tq, &Tk, &dh, &ld, &off) != 7) return 2;
      AttnFwdProblem p{base, base, base, nullptr, base + off, nullptr, B, H, Tq, Tk, dh, ld, ld, ld, ld, 0.f, 0, VMC_BF16};
      printf("%s\n", kname(attn_fwd_route(p)));
    } else if (!strcmp(kind, "bwd")) {
      int B, H, Tq, Tk, dh, ld, lddq, ldo, goff, ooff;
      if (scanf("%d %d %d %d %d %d %d %d %d %d", &B, &H, &Tq, &Tk, &dh, &ld, &lddq, &ldo, &goff, &ooff) != 10) return 2;
      AttnBwdProblem p{base, base, base, nullptr, base + ooff, base, (const float*)base, base + goff, base + goff, base + goff,
                       B, H, Tq, Tk, dh, ld, ld, ld, ldo, lddq, ld, ld, 0.f, 0, base, attn_bwd_workspace_bytes(B, H, Tq), VMC_BF16};
      const AttnPlan pl = attn_bwd_route(p);
      printf("%s %d %d\n", kname(pl), pl.block, pl.rs);
    } else {
      return 2;
    }
  }
  return 0;
}
