// Per-item self-test of the field and scalar primitives (TEST INFRASTRUCTURE: the cross-check build's k_fe_selftest and the host
// twin hd_fe_selftest in tests/hostcheck/device_src_host.cpp include this one function, so the device and the g++ build of the
// device sources run literally the same dispatcher — on the device with the KYB_ASM_COLUMNS product columns, the asm doublings and
// the 64-bit additions, on the host with the overflow-checked C branches).  tests/test_gpu_field_bounds.py compares the two limb
// for limb and tests/field_reference.py checks the values at each primitive's documented bounds.
//
// An item: three operand slots a, b, c of 16 words (RAW limbs in words 0..9 — not bytes, so loose limbs reach the primitive as
// they are; 32-bit words for the scalar ops and fe_from_words), a 32-bit parameter, and 16 output words.  Words of the output
// an op does not write stay 0.
#pragma once
#include "fe25519.h"
#include "fe_invert_gcd.h"
#include "sc25519.h"
#include "ge25519.h"

namespace kyb {

enum fe_selftest_op : uint32_t {
  FT_MUL = 0, FT_MUL_B6, FT_SQ, FT_SQ_B2, FT_SQN,                        // param: n of fe_sqn
  FT_ADD = 5, FT_ADDW, FT_SUB, FT_SUBW, FT_SUB4, FT_NEG,
  FT_REDUCE_WEAK = 11, FT_CANON, FT_TO_WORDS, FT_FROM_WORDS, FT_IS_NEGATIVE, FT_IS_NONZERO,
  FT_INVERT = 17, FT_POW22523, FT_INVERT_GCD,
  FT_SELECT = 20, FT_CSWAP_F, FT_CSWAP_G,                                // param: c; the two halves of fe_cswap's result
  FT_FROM_REF10 = 23, FT_TO_REF10,                                       // a: ten signed limbs / out: ten signed limbs
  SC_REDUCE512 = 25, SC_REDUCE256, SC_MULADD, SC_RECODE, SC_POW_MOD8L,   // SC_RECODE: out[8] = top; SC_POW_MOD8L: x = a[0], e = param, out[8] = neg
  FE_SELFTEST_OPS = 30
};

KYB_HD void fe_selftest_item(uint32_t op, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t param, uint32_t* out) {
  fe f, g, h;
  KYB_UNROLL for (int i = 0; i < 10; ++i) { f.v[i] = a[i]; g.v[i] = b[i]; h.v[i] = 0; }
  uint32_t o[16];
  KYB_UNROLL for (int i = 0; i < 16; ++i) o[i] = 0;
  bool limbs = true;                                                     // the result is h (ten limbs), else o
  switch (op) {
    case FT_MUL: fe_mul(h, f, g); break;
    case FT_MUL_B6: fe_mul_b6(h, f, g); break;
    case FT_SQ: fe_sq(h, f); break;
    case FT_SQ_B2: fe_sq_b2(h, f); break;
    case FT_SQN: fe_sqn(h, f, (int)param); break;
    case FT_ADD: fe_add(h, f, g); break;
    case FT_ADDW: fe_addw(h, f, g); break;
    case FT_SUB: fe_sub(h, f, g); break;
    case FT_SUBW: fe_subw(h, f, g); break;
    case FT_SUB4: fe_sub4(h, f, g); break;
    case FT_NEG: fe_neg(h, f); break;
    case FT_REDUCE_WEAK: fe_reduce_weak(h, f); break;
    case FT_CANON: fe_canon(h, f); break;
    case FT_TO_WORDS: fe_to_words(o, f); limbs = false; break;
    case FT_FROM_WORDS: fe_from_words(h, a); break;
    case FT_IS_NEGATIVE: o[0] = fe_is_negative(f); limbs = false; break;
    case FT_IS_NONZERO: o[0] = fe_is_nonzero(f); limbs = false; break;
    case FT_INVERT: fe_invert(h, f); break;
    case FT_POW22523: fe_pow22523(h, f); break;
    case FT_INVERT_GCD: fe_invert_gcd(h, f); break;
    case FT_SELECT: fe_select(h, f, g, param); break;
    case FT_CSWAP_F: fe_cswap(f, g, param); fe_copy(h, f); break;
    case FT_CSWAP_G: fe_cswap(f, g, param); fe_copy(h, g); break;
    case FT_FROM_REF10: {
      int32_t s[10];
      KYB_UNROLL for (int i = 0; i < 10; ++i) s[i] = (int32_t)a[i];
      fe_from_ref10(h, s);
      break;
    }
    case FT_TO_REF10: {
      int32_t s[10];
      fe_to_ref10(s, f);
      KYB_UNROLL for (int i = 0; i < 10; ++i) o[i] = (uint32_t)s[i];
      limbs = false;
      break;
    }
    case SC_REDUCE512: sc_reduce512(o, a); limbs = false; break;
    case SC_REDUCE256: sc_reduce256(o, a); limbs = false; break;
    case SC_MULADD: sc_muladd(o, a, b, c); limbs = false; break;
    case SC_RECODE: {
      sc_digits d;
      sc_recode(d, a);
      KYB_UNROLL for (int i = 0; i < 8; ++i) o[i] = d.w[i];
      o[8] = d.top;
      limbs = false;
      break;
    }
    case SC_POW_MOD8L: {
      uint32_t neg;
      sc_pow_mod8L_signed(o, neg, a[0], param);
      o[8] = neg;
      limbs = false;
      break;
    }
    default: break;
  }
  if (limbs) KYB_UNROLL for (int i = 0; i < 10; ++i) o[i] = h.v[i];
  KYB_UNROLL for (int i = 0; i < 16; ++i) out[i] = o[i];
}

}  // namespace kyb
