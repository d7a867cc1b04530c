// extern "C" entry points declared in include/kyber_ed25519.h.  Textually included at the end of
// engine.hip: they use its anonymous-namespace contexts (Ctx, launch_*, run_host_batch).  Every entry resolves the
// calling thread's context (kyb_ctx_set_current, default = the kyb_init context) and makes its device current.
extern "C" {

int kyb_abi_version(void) { return KYB_ABI_VERSION; }
int kyb_init(int device) { return do_init(device, true); }
int kyb_init_no_table(int device) { return do_init(device, false); }

void kyb_shutdown(void) {
  Ctx* c;
  { std::lock_guard<std::mutex> lk(g_reg_mu); c = g_default; }
  if (c != nullptr) ctx_delete(c);
}

const char* kyb_last_error(void) { return g_err.c_str(); }

int kyb_device_info(char* name, size_t name_cap, int* compute_units, size_t* workspace_bytes) {
  ENTER();
  if (name && name_cap) snprintf(name, name_cap, "%s", g.name);
  if (compute_units) *compute_units = g.cus;
  if (workspace_bytes) *workspace_bytes = g.ws_bytes;
  return KYB_OK;
}

int kyb_sync(void* stream) {
  ENTER();
  HIPCK(hipStreamSynchronize(pick(g, stream)));
  return KYB_OK;
}

int kyb_stream_release(void* stream) {
  ENTER();
  if (!stream) return fail(KYB_E_BAD_ARG, "the engine's own stream cannot be released");
  std::lock_guard<std::mutex> launch_lock(g.launch_mu);
  for (size_t i = 0; i < g.res.size(); ++i)
    if (g.res[i]->stream == caller_stream(stream) && !g.res[i]->own) {
      free_slot(g, g.res[i]);                 // waits for the slot's last launch (an event: the stream itself may be gone already)
      g.res.erase(g.res.begin() + (long)i);
      break;
    }
  return KYB_OK;
}

int kyb_base_table_export_dev(void* dst_dev, void* stream) {
  ENTER(); REQUIRE_TABLE();
  if (!dst_dev) return fail(KYB_E_BAD_ARG, "null destination");
  HIPCK(hipMemcpyAsync(dst_dev, g.table, KYB_BASE_TABLE_BYTES, hipMemcpyDeviceToDevice, pick(g, stream)));
  return KYB_OK;
}
int kyb_base_table_import_dev(const void* src_dev, void* stream) {
  ENTER();
  if (!src_dev) return fail(KYB_E_BAD_ARG, "null source");
  g.table_ready = false;
  HIPCK(hipMemcpyAsync(g.table, src_dev, KYB_BASE_TABLE_BYTES, hipMemcpyDeviceToDevice, pick(g, stream)));
  int rc = table_validate(g, pick(g, stream));      // the image carries its own checksum: a bad broadcast is refused here
  if (rc) return rc;
  g.table_ready = true;
  return KYB_OK;
}
int kyb_base_table_export(uint8_t* dst_host) {
  ENTER(); REQUIRE_TABLE();
  if (!dst_host) return fail(KYB_E_BAD_ARG, "null destination");
  HIPCK(hipMemcpy(dst_host, g.table, KYB_BASE_TABLE_BYTES, hipMemcpyDeviceToHost));
  return KYB_OK;
}
int kyb_base_table_import(const uint8_t* src_host) {
  ENTER();
  if (!src_host) return fail(KYB_E_BAD_ARG, "null source");
  g.table_ready = false;
  HIPCK(hipMemcpy(g.table, src_host, KYB_BASE_TABLE_BYTES, hipMemcpyHostToDevice));
  int rc = table_validate(g, g.stream);
  if (rc) return rc;
  g.table_ready = true;
  return KYB_OK;
}

// ---- device-pointer API ----
int kyb_mul_base_batch_dev(const uint8_t* scalars, size_t n, uint8_t* out_enc, int32_t* out_ext, void* stream) {
  ENTER(); REQUIRE_TABLE();
  if (n && (!scalars || (!out_enc && !out_ext))) return fail(KYB_E_BAD_ARG, "null buffer");
  if (!aligned16(scalars) || !aligned16(out_enc) || !aligned16(out_ext)) return fail(KYB_E_BAD_ARG, "device buffers must be 16-byte aligned");
  return drained(launch_mul_base(g, scalars, n, out_enc, out_ext, pick(g, stream)));
}
int kyb_mul_batch_dev(const uint8_t* scalars, const uint8_t* pts_enc, const int32_t* pts_ext, size_t n,
                      uint8_t* out_enc, int32_t* out_ext, uint8_t* ok, void* stream) {
  ENTER();
  if (n && (!scalars || (!out_enc && !out_ext))) return fail(KYB_E_BAD_ARG, "null buffer");
  if (n && ((pts_enc == nullptr) == (pts_ext == nullptr))) return fail(KYB_E_BAD_ARG, "give exactly one of pts_enc / pts_ext");
  if (!aligned16(scalars) || !aligned16(pts_enc) || !aligned16(pts_ext) || !aligned16(out_enc) || !aligned16(out_ext))
    return fail(KYB_E_BAD_ARG, "device buffers must be 16-byte aligned");
  return drained(launch_mul(g, scalars, pts_enc, pts_ext, n, out_enc, out_ext, ok, pick(g, stream)));
}
int kyb_add_batch_dev(const int32_t* a_ext, const int32_t* b_ext, size_t n, int32_t* out_ext, int subtract, void* stream) {
  ENTER();
  if (n == 0) return KYB_OK;
  if (!a_ext || !b_ext || !out_ext) return fail(KYB_E_BAD_ARG, "null buffer");
  if (!aligned16(a_ext) || !aligned16(b_ext) || !aligned16(out_ext)) return fail(KYB_E_BAD_ARG, "device buffers must be 16-byte aligned");
  LAUNCHCK(launch::add(pick(g, stream), a_ext, b_ext, n, out_ext, subtract));
  return KYB_OK;
}
int kyb_encode_batch_dev(const int32_t* pts_ext, size_t n, uint8_t* out_enc, void* stream) {
  ENTER();
  if (n == 0) return KYB_OK;
  if (!pts_ext || !out_enc) return fail(KYB_E_BAD_ARG, "null buffer");
  if (!aligned16(pts_ext) || !aligned16(out_enc)) return fail(KYB_E_BAD_ARG, "device buffers must be 16-byte aligned");
  return drained(launch_encode(g, pts_ext, n, out_enc, pick(g, stream)));
}
int kyb_decode_batch_dev(const uint8_t* enc, size_t n, int32_t* out_ext, uint8_t* ok, void* stream) {
  ENTER();
  if (n == 0) return KYB_OK;
  if (!enc || !out_ext) return fail(KYB_E_BAD_ARG, "null buffer");
  if (!aligned16(enc) || !aligned16(out_ext)) return fail(KYB_E_BAD_ARG, "device buffers must be 16-byte aligned");
  hipStream_t st = pick(g, stream);
  if (n <= coop_lim(g, g.opt_coop_decode_max)) {      // small batch: one item per wavefront
    ProfScope ps(g, st, KID_DECODE_COOP);
    LAUNCHCK(launch::decode_coop(st, enc, n, out_ext, ok, false, take_done_flag(g, st, n)));
    return KYB_OK;
  }
  { ProfScope ps(g, st, KID_DECODE); LAUNCHCK(launch::decode(st, enc, n, out_ext, ok)); }
  return KYB_OK;
}
int kyb_schnorr_sign_keyed_batch_dev(const uint8_t* x, const uint8_t* pubs, const uint8_t* k, const uint8_t* msgs, const uint32_t* msg_off, size_t n,
                                     uint8_t* sig, void* stream) {
  ENTER(); REQUIRE_TABLE();
  if (n == 0) return KYB_OK;
  if (!x || !k || !msg_off || !sig) return fail(KYB_E_BAD_ARG, "null buffer");
  if (!aligned16(x) || !aligned16(k) || !aligned16(sig) || !aligned16(pubs)) return fail(KYB_E_BAD_ARG, "device buffers must be 16-byte aligned");
  return drained(launch_sign(g, x, k, pubs, msgs, msg_off, n, sig, pick(g, stream)));
}
int kyb_schnorr_sign_batch_dev(const uint8_t* x, const uint8_t* k, const uint8_t* msgs, const uint32_t* msg_off, size_t n, uint8_t* sig, void* stream) {
  return kyb_schnorr_sign_keyed_batch_dev(x, nullptr, k, msgs, msg_off, n, sig, stream);
}

// ---- host-pointer API: stage through one device buffer, run on the engine stream, copy back ----
int kyb_mul_base_batch(const uint8_t* scalars, size_t n, uint8_t* out_enc, int32_t* out_ext) {
  ENTER(); REQUIRE_TABLE();
  if (n == 0) return KYB_OK;
  if (!scalars || (!out_enc && !out_ext)) return fail(KYB_E_BAD_ARG, "null buffer");
  const HostArr arrs[3] = {{scalars, nullptr, 32, true}, {nullptr, out_enc, 32}, {nullptr, out_ext, 160}};      // the scalars may be private keys or nonces
  return run_host_batch(g, n, arrs, 3, [&](hipStream_t st, size_t cn, uint8_t** d) {
    return drained(launch_mul_base(g, d[0], cn, d[1], reinterpret_cast<int32_t*>(d[2]), st));
  });
}
namespace {
int mul_batch_host(const uint8_t* scalars, const uint8_t* pts_enc, const int32_t* pts_ext, size_t n, uint8_t* out_enc, int32_t* out_ext, uint8_t* ok,
                   bool multipliers_public) {
  ENTER();
  if (n == 0) return KYB_OK;
  if (!scalars || (!out_enc && !out_ext)) return fail(KYB_E_BAD_ARG, "null buffer");
  if ((pts_enc == nullptr) == (pts_ext == nullptr)) return fail(KYB_E_BAD_ARG, "give exactly one of pts_enc / pts_ext");
  const bool sec = !multipliers_public;                                                                                     // the scalars may be DH secrets, and then s*P is the shared secret
  const HostArr arrs[6] = {{scalars, nullptr, 32, sec}, {pts_enc, nullptr, 32}, {pts_ext, nullptr, 160},
                           {nullptr, out_enc, 32, sec}, {nullptr, out_ext, 160, sec}, {nullptr, ok, 1}};
  // leading zero bits common to all scalars of a small call (exact: the canonical-range test needs every scalar looked at); public multipliers that
  // are all short take a short ladder (launch_mul)
  const int skip_hint = (n <= 64 && pts_ext != nullptr) ? common_leading_zero_bits(scalars, n, 256) : 0;
  return run_host_batch(g, n, arrs, 6, [&](hipStream_t st, size_t cn, uint8_t** d) {
    return drained(launch_mul(g, d[0], d[1], reinterpret_cast<const int32_t*>(d[2]), cn, d[3], reinterpret_cast<int32_t*>(d[4]), d[5], st, skip_hint, multipliers_public));
  });
}
}  // namespace
int kyb_mul_batch(const uint8_t* scalars, const uint8_t* pts_enc, const int32_t* pts_ext, size_t n,
                  uint8_t* out_enc, int32_t* out_ext, uint8_t* ok) {
  return mul_batch_host(scalars, pts_enc, pts_ext, n, out_enc, out_ext, ok, false);
}
int kyb_mul_public_batch(const uint8_t* scalars, const uint8_t* pts_enc, const int32_t* pts_ext, size_t n,
                         uint8_t* out_enc, int32_t* out_ext, uint8_t* ok) {
  return mul_batch_host(scalars, pts_enc, pts_ext, n, out_enc, out_ext, ok, true);
}
int kyb_add_batch(const int32_t* a_ext, const int32_t* b_ext, size_t n, int32_t* out_ext, int subtract) {
  ENTER();
  if (n == 0) return KYB_OK;
  if (!a_ext || !b_ext || !out_ext) return fail(KYB_E_BAD_ARG, "null buffer");
  HostCall c(g);
  const int a = c.in(a_ext, 160 * n), b = c.in(b_ext, 160 * n), o = c.out(out_ext, 160 * n);
  return c.run([&](hipStream_t st) { return kyb_add_batch_dev(c.dev<int32_t>(a), c.dev<int32_t>(b), n, c.dev<int32_t>(o), subtract, st); });
}
int kyb_encode_batch(const int32_t* pts_ext, size_t n, uint8_t* out_enc) {
  ENTER();
  if (n == 0) return KYB_OK;
  if (!pts_ext || !out_enc) return fail(KYB_E_BAD_ARG, "null buffer");
  HostCall c(g);
  const int p = c.in(pts_ext, 160 * n), e = c.out(out_enc, 32 * n);
  return c.run([&](hipStream_t st) { return kyb_encode_batch_dev(c.dev<int32_t>(p), n, c.dev(e), st); });
}
int kyb_decode_batch(const uint8_t* enc, size_t n, int32_t* out_ext, uint8_t* ok) {
  ENTER();
  if (n == 0) return KYB_OK;
  if (!enc || !out_ext) return fail(KYB_E_BAD_ARG, "null buffer");
  HostCall c(g);
  const int e = c.in(enc, 32 * n), p = c.out(out_ext, 160 * n), k = c.out(ok, n);
  return c.run([&](hipStream_t st) { return kyb_decode_batch_dev(c.dev(e), n, c.dev<int32_t>(p), c.dev(k), st); });
}
int kyb_schnorr_sign_keyed_batch(const uint8_t* x, const uint8_t* pubs, const uint8_t* k, const uint8_t* msgs, const uint32_t* msg_off, size_t n, uint8_t* sig) {
  ENTER(); REQUIRE_TABLE();
  if (n == 0) return KYB_OK;
  if (!x || !k || !msg_off || !sig) return fail(KYB_E_BAD_ARG, "null buffer");
  size_t mbytes;
  { int rc = check_messages(msgs, msg_off, n, &mbytes); if (rc) return rc; }
  HostCall c(g);
  c.secret();
  const int ix = c.in(x, 32 * n), ik = c.in(k, 32 * n), ip = c.in(pubs, 32 * n), im = c.in(msgs ? msgs : x, mbytes, 16), io = c.in(msg_off, 4 * (n + 1)),
            is = c.out(sig, 64 * n);
  return c.run([&](hipStream_t st) { return drained(launch_sign(g, c.dev(ix), c.dev(ik), c.dev(ip), c.dev(im), c.dev<uint32_t>(io), n, c.dev(is), st)); });
}
int kyb_schnorr_sign_batch(const uint8_t* x, const uint8_t* k, const uint8_t* msgs, const uint32_t* msg_off, size_t n, uint8_t* sig) {
  return kyb_schnorr_sign_keyed_batch(x, nullptr, k, msgs, msg_off, n, sig);
}

namespace {
int eddsa_sign_dev(const uint8_t* seeds, const uint8_t* pubs_in, const uint8_t* msgs, const uint32_t* msg_off, size_t n, uint8_t* sig, uint8_t* pub_out, void* stream) {
  ENTER(); REQUIRE_TABLE();
  if (n == 0) return KYB_OK;
  if (!seeds || !msg_off || !sig) return fail(KYB_E_BAD_ARG, "null buffer");
  if (!aligned16(seeds) || !aligned16(sig) || !aligned16(pubs_in) || !aligned16(pub_out)) return fail(KYB_E_BAD_ARG, "device buffers must be 16-byte aligned");
  return drained(launch_eddsa_sign(g, seeds, pubs_in, msgs, msg_off, n, sig, pub_out, pick(g, stream)));
}
int eddsa_sign_host(const uint8_t* seeds, const uint8_t* pubs_in, const uint8_t* msgs, const uint32_t* msg_off, size_t n, uint8_t* sig, uint8_t* pub_out) {
  ENTER(); REQUIRE_TABLE();
  if (n == 0) return KYB_OK;
  if (!seeds || !msg_off || !sig) return fail(KYB_E_BAD_ARG, "null buffer");
  size_t mbytes;
  { int rc = check_messages(msgs, msg_off, n, &mbytes); if (rc) return rc; }
  HostCall c(g);
  c.secret();
  const int is = c.in(seeds, 32 * n), im = c.in(msgs ? msgs : seeds, mbytes, 16), io = c.in(msg_off, 4 * (n + 1)), ig = c.out(sig, 64 * n),
            ip = c.inout(pubs_in, pubs_in ? nullptr : pub_out, 32 * n);
  return c.run([&](hipStream_t st) {
    return drained(launch_eddsa_sign(g, c.dev(is), pubs_in ? c.dev(ip) : nullptr, c.dev(im), c.dev<uint32_t>(io), n, c.dev(ig), pubs_in ? nullptr : c.dev(ip), st));
  });
}
}  // namespace
int kyb_eddsa_sign_batch_dev(const uint8_t* seeds, const uint8_t* msgs, const uint32_t* msg_off, size_t n, uint8_t* sig, uint8_t* pub, void* stream) {
  return eddsa_sign_dev(seeds, nullptr, msgs, msg_off, n, sig, pub, stream);
}
int kyb_eddsa_sign_batch(const uint8_t* seeds, const uint8_t* msgs, const uint32_t* msg_off, size_t n, uint8_t* sig, uint8_t* pub) {
  return eddsa_sign_host(seeds, nullptr, msgs, msg_off, n, sig, pub);
}
int kyb_eddsa_sign_keyed_batch_dev(const uint8_t* seeds, const uint8_t* pubs, const uint8_t* msgs, const uint32_t* msg_off, size_t n, uint8_t* sig, void* stream) {
  if (n && !pubs) return fail(KYB_E_BAD_ARG, "null buffer");
  return eddsa_sign_dev(seeds, pubs, msgs, msg_off, n, sig, nullptr, stream);
}
int kyb_eddsa_sign_keyed_batch(const uint8_t* seeds, const uint8_t* pubs, const uint8_t* msgs, const uint32_t* msg_off, size_t n, uint8_t* sig) {
  if (n && !pubs) return fail(KYB_E_BAD_ARG, "null buffer");
  return eddsa_sign_host(seeds, pubs, msgs, msg_off, n, sig, nullptr);
}

int kyb_verify_batch_dev(const uint8_t* pubs, const uint8_t* msgs, const uint32_t* msg_off, const uint8_t* sigs, size_t n, int flavor,
                         uint8_t* status, void* stream) {
  ENTER(); REQUIRE_TABLE();
  if (n == 0) return KYB_OK;
  if (!pubs || !msg_off || !sigs || !status) return fail(KYB_E_BAD_ARG, "null buffer");
  if (flavor != 0 && flavor != 1) return fail(KYB_E_BAD_ARG, "flavor: 0 = eddsa check order, 1 = schnorr check order");
  if (!aligned16(pubs) || !aligned16(sigs)) return fail(KYB_E_BAD_ARG, "device buffers must be 16-byte aligned");
  return drained(launch_verify(g, pubs, msgs, msg_off, sigs, n, flavor, status, pick(g, stream)));
}
int kyb_verify_batch(const uint8_t* pubs, const uint8_t* msgs, const uint32_t* msg_off, const uint8_t* sigs, size_t n, int flavor, uint8_t* status) {
  ENTER(); REQUIRE_TABLE();
  if (n == 0) return KYB_OK;
  if (!pubs || !msg_off || !sigs || !status) return fail(KYB_E_BAD_ARG, "null buffer");
  if (flavor != 0 && flavor != 1) return fail(KYB_E_BAD_ARG, "flavor: 0 = eddsa check order, 1 = schnorr check order");
  size_t mbytes;
  { int rc = check_messages(msgs, msg_off, n, &mbytes); if (rc) return rc; }
  HostCall c(g);
  const int ip = c.in(pubs, 32 * n), is = c.in(sigs, 64 * n), im = c.in(msgs ? msgs : pubs, mbytes, 16), io = c.in(msg_off, 4 * (n + 1)), it = c.out(status, n);
  return c.run([&](hipStream_t st) { return drained(launch_verify(g, c.dev(ip), c.dev(im), c.dev<uint32_t>(io), c.dev(is), n, flavor, c.dev(it), st)); });
}

// schnorr::verify / eddsa::verify (schnorr_sig.rs:114-127, eddsa_sig.rs:216-...): the public keys as the Points the callers hold
int kyb_verify_points_batch_dev(const int32_t* pubs_ext, const uint8_t* msgs, const uint32_t* msg_off, const uint8_t* sigs, size_t n, int flavor,
                                uint8_t* status, void* stream) {
  ENTER(); REQUIRE_TABLE();
  if (n == 0) return KYB_OK;
  if (!pubs_ext || !msg_off || !sigs || !status) return fail(KYB_E_BAD_ARG, "null buffer");
  if (flavor != 0 && flavor != 1) return fail(KYB_E_BAD_ARG, "flavor: 0 = eddsa check order, 1 = schnorr check order");
  if (!aligned16(pubs_ext) || !aligned16(sigs)) return fail(KYB_E_BAD_ARG, "device buffers must be 16-byte aligned");
  return drained(launch_verify(g, nullptr, msgs, msg_off, sigs, n, flavor, status, pick(g, stream), pubs_ext));
}
int kyb_verify_points_batch(const int32_t* pubs_ext, const uint8_t* msgs, const uint32_t* msg_off, const uint8_t* sigs, size_t n, int flavor, uint8_t* status) {
  ENTER(); REQUIRE_TABLE();
  if (n == 0) return KYB_OK;
  if (!pubs_ext || !msg_off || !sigs || !status) return fail(KYB_E_BAD_ARG, "null buffer");
  if (flavor != 0 && flavor != 1) return fail(KYB_E_BAD_ARG, "flavor: 0 = eddsa check order, 1 = schnorr check order");
  size_t mbytes;
  { int rc = check_messages(msgs, msg_off, n, &mbytes); if (rc) return rc; }
  HostCall c(g);
  const int ip = c.in(pubs_ext, 160 * n), is = c.in(sigs, 64 * n), im = c.in(msgs ? msgs : reinterpret_cast<const uint8_t*>(pubs_ext), mbytes, 16), io = c.in(msg_off, 4 * (n + 1)),
            it = c.out(status, n);
  return c.run([&](hipStream_t st) { return drained(launch_verify(g, nullptr, c.dev(im), c.dev<uint32_t>(io), c.dev(is), n, flavor, c.dev(it), st, c.dev<int32_t>(ip))); });
}

int kyb_pubpoly_eval_batch_dev(const int32_t* commits_ext, size_t t, const uint32_t* indices, size_t n, uint32_t max_index,
                               uint8_t* out_enc, int32_t* out_ext, void* stream) {
  ENTER();
  if (n == 0) return KYB_OK;
  if (!commits_ext || !indices || (!out_enc && !out_ext) || t == 0 || t > (1u << 20)) return fail(KYB_E_BAD_ARG, "bad argument");
  if (max_index == 0xffffffffu) return fail(KYB_E_BAD_ARG, "index + 1 must fit 32 bits");
  if (!aligned16(commits_ext) || !aligned16(out_enc) || !aligned16(out_ext)) return fail(KYB_E_BAD_ARG, "device buffers must be 16-byte aligned");
  return drained(launch_poly_eval(g, commits_ext, t, indices, n, max_index, out_enc, out_ext, pick(g, stream)));
}
int kyb_pubpoly_eval_batch(const int32_t* commits_ext, size_t t, const uint32_t* indices, size_t n, uint8_t* out_enc, int32_t* out_ext) {
  ENTER();
  if (n == 0) return KYB_OK;
  if (!commits_ext || !indices || (!out_enc && !out_ext) || t == 0 || t > (1u << 20)) return fail(KYB_E_BAD_ARG, "bad argument");
  uint32_t mx = 0;
  for (size_t i = 0; i < n; ++i) mx = indices[i] > mx ? indices[i] : mx;
  if (mx == 0xffffffffu) return fail(KYB_E_BAD_ARG, "index + 1 must fit 32 bits");
  HostCall c(g);
  const int ic = c.in(commits_ext, 160 * t), ii = c.in(indices, 4 * n), ie = c.out(out_enc, 32 * n), ix = c.out(out_ext, 160 * n);
  return c.run([&](hipStream_t st) { return drained(launch_poly_eval(g, c.dev<int32_t>(ic), t, c.dev<uint32_t>(ii), n, mx, c.dev(ie), c.dev<int32_t>(ix), st)); });
}
int kyb_lincomb_batch_dev(const uint8_t* scalars, const uint8_t* pts_enc, const int32_t* pts_ext, int shared_points,
                          size_t m, size_t t, uint8_t* out_enc, int32_t* out_ext, uint8_t* ok, void* stream) {
  ENTER();
  if (m == 0) return KYB_OK;
  if (t == 0 || t > (size_t(1) << 24) || m > (size_t(1) << 28) / t) return fail(KYB_E_BAD_ARG, "m * t out of range");
  if (!scalars || (!out_enc && !out_ext)) return fail(KYB_E_BAD_ARG, "null buffer");
  if ((pts_enc == nullptr) == (pts_ext == nullptr)) return fail(KYB_E_BAD_ARG, "give exactly one of pts_enc / pts_ext");
  if (!aligned16(scalars) || !aligned16(pts_enc) || !aligned16(pts_ext) || !aligned16(out_enc) || !aligned16(out_ext))
    return fail(KYB_E_BAD_ARG, "device buffers must be 16-byte aligned");
  return drained(launch_lincomb(g, scalars, pts_enc, pts_ext, shared_points != 0, m, t, ok, out_enc, out_ext, pick(g, stream)));
}
int kyb_lincomb_batch(const uint8_t* scalars, const uint8_t* pts_enc, const int32_t* pts_ext, int shared_points,
                      size_t m, size_t t, uint8_t* out_enc, int32_t* out_ext, uint8_t* ok) {
  ENTER();
  if (m == 0) return KYB_OK;
  if (t == 0 || t > (size_t(1) << 24) || m > (size_t(1) << 28) / t) return fail(KYB_E_BAD_ARG, "m * t out of range");
  if (!scalars || (!out_enc && !out_ext)) return fail(KYB_E_BAD_ARG, "null buffer");
  if ((pts_enc == nullptr) == (pts_ext == nullptr)) return fail(KYB_E_BAD_ARG, "give exactly one of pts_enc / pts_ext");
  const size_t n = m * t, np = shared_points ? t : n;
  HostCall c(g);
  const int is = c.in(scalars, 32 * n), ipe = c.in(pts_enc, 32 * np), ipx = c.in(pts_ext, 160 * np), ie = c.out(out_enc, 32 * m), ix = c.out(out_ext, 160 * m),
            ik = c.out(ok, np);
  return c.run([&](hipStream_t st) {
    return drained(launch_lincomb(g, c.dev(is), c.dev(ipe), c.dev<int32_t>(ipx), shared_points != 0, m, t, c.dev(ik), c.dev(ie), c.dev<int32_t>(ix), st));
  });
}
// PriPoly::eval / shares (poly.rs:133-152): m secret polynomials of t coefficients evaluated at k public share indices
int kyb_pripoly_eval_batch_dev(const uint8_t* coeffs, size_t m, size_t t, const uint32_t* indices, size_t k, uint8_t* out_shares, void* stream) {
  ENTER();
  if (m == 0 || k == 0) return KYB_OK;
  if (!coeffs || !indices || !out_shares || t == 0 || t > (size_t(1) << 24) || m > (size_t(1) << 28) / t || k > (size_t(1) << 28) / m) return fail(KYB_E_BAD_ARG, "bad argument");
  if (!aligned16(coeffs) || !aligned16(out_shares)) return fail(KYB_E_BAD_ARG, "device buffers must be 16-byte aligned");
  return drained(launch_pripoly_eval(g, coeffs, m, t, indices, k, out_shares, pick(g, stream)));
}
int kyb_pripoly_eval_batch(const uint8_t* coeffs, size_t m, size_t t, const uint32_t* indices, size_t k, uint8_t* out_shares) {
  ENTER();
  if (m == 0 || k == 0) return KYB_OK;
  if (!coeffs || !indices || !out_shares || t == 0 || t > (size_t(1) << 24) || m > (size_t(1) << 28) / t || k > (size_t(1) << 28) / m) return fail(KYB_E_BAD_ARG, "bad argument");
  for (size_t i = 0; i < k; ++i) if (indices[i] == 0xffffffffu) return fail(KYB_E_BAD_ARG, "index + 1 must fit 32 bits");
  HostCall c(g);
  c.secret();                                          // coefficients and shares are secrets: staging wiped on every exit path
  const int ic = c.in(coeffs, 32 * m * t), ii = c.in(indices, 4 * k), io = c.out(out_shares, 32 * m * k);
  return c.run([&](hipStream_t st) { return kyb_pripoly_eval_batch_dev(c.dev(ic), m, t, c.dev<uint32_t>(ii), k, c.dev(io), st); });
}
// the Lagrange coefficients at 0 of m share sets of t public indices each (recover_commit, poly.rs:580-594)
int kyb_lagrange_coeffs_batch_dev(const uint32_t* indices, size_t m, size_t t, uint8_t* out_scalars, void* stream) {
  ENTER();
  if (m == 0 || t == 0) return KYB_OK;
  if (!indices || !out_scalars || t > (size_t(1) << 20) || m > (size_t(1) << 28) / t) return fail(KYB_E_BAD_ARG, "bad argument");
  if (!aligned16(out_scalars)) return fail(KYB_E_BAD_ARG, "device buffers must be 16-byte aligned");
  LAUNCHCK(launch::lagrange_at_zero(pick(g, stream), indices, m, t, out_scalars));
  return KYB_OK;
}
int kyb_lagrange_coeffs_batch(const uint32_t* indices, size_t m, size_t t, uint8_t* out_scalars) {
  ENTER();
  if (m == 0 || t == 0) return KYB_OK;
  if (!indices || !out_scalars || t > (size_t(1) << 20) || m > (size_t(1) << 28) / t) return fail(KYB_E_BAD_ARG, "bad argument");
  for (size_t i = 0; i < m * t; ++i) if (indices[i] == 0xffffffffu) return fail(KYB_E_BAD_ARG, "index + 1 must fit 32 bits");
  HostCall c(g);
  const int ii = c.in(indices, 4 * m * t), io = c.out(out_scalars, 32 * m * t);
  return c.run([&](hipStream_t st) { return kyb_lagrange_coeffs_batch_dev(c.dev<uint32_t>(ii), m, t, c.dev(io), st); });
}
int kyb_lincomb_public_batch_dev(const uint8_t* scalars, const uint8_t* pts_enc, const int32_t* pts_ext, int shared_points,
                                 size_t m, size_t t, uint8_t* out_enc, int32_t* out_ext, uint8_t* ok, void* stream) {
  ENTER();
  if (m == 0) return KYB_OK;
  if (t == 0 || t > (size_t(1) << 24) || m > (size_t(1) << 28) / t) return fail(KYB_E_BAD_ARG, "m * t out of range");
  if (!scalars || (!out_enc && !out_ext)) return fail(KYB_E_BAD_ARG, "null buffer");
  if ((pts_enc == nullptr) == (pts_ext == nullptr)) return fail(KYB_E_BAD_ARG, "give exactly one of pts_enc / pts_ext");
  if (!aligned16(scalars) || !aligned16(pts_enc) || !aligned16(pts_ext) || !aligned16(out_enc) || !aligned16(out_ext))
    return fail(KYB_E_BAD_ARG, "device buffers must be 16-byte aligned");
  return drained(launch_lincomb_public(g, scalars, pts_enc, pts_ext, shared_points != 0, m, t, ok, out_enc, out_ext, pick(g, stream)));
}
int kyb_lincomb_public_batch(const uint8_t* scalars, const uint8_t* pts_enc, const int32_t* pts_ext, int shared_points,
                             size_t m, size_t t, uint8_t* out_enc, int32_t* out_ext, uint8_t* ok) {
  ENTER();
  if (m == 0) return KYB_OK;
  if (t == 0 || t > (size_t(1) << 24) || m > (size_t(1) << 28) / t) return fail(KYB_E_BAD_ARG, "m * t out of range");
  if (!scalars || (!out_enc && !out_ext)) return fail(KYB_E_BAD_ARG, "null buffer");
  if ((pts_enc == nullptr) == (pts_ext == nullptr)) return fail(KYB_E_BAD_ARG, "give exactly one of pts_enc / pts_ext");
  const size_t n = m * t, np = shared_points ? t : n;
  HostCall c(g);
  const int is = c.in(scalars, 32 * n), ipe = c.in(pts_enc, 32 * np), ipx = c.in(pts_ext, 160 * np), ie = c.out(out_enc, 32 * m), ix = c.out(out_ext, 160 * m),
            ik = c.out(ok, np);
  return c.run([&](hipStream_t st) {
    return drained(launch_lincomb_public(g, c.dev(is), c.dev(ipe), c.dev<int32_t>(ipx), shared_points != 0, m, t, c.dev(ik), c.dev(ie), c.dev<int32_t>(ix), st));
  });
}
int kyb_pubpoly_eval_multi_batch_dev(const int32_t* commits_ext, size_t t, size_t m, const uint32_t* indices, size_t k, uint32_t max_index,
                                     uint8_t* out_enc, int32_t* out_ext, void* stream) {
  ENTER();
  if (m == 0 || k == 0) return KYB_OK;
  if (!commits_ext || !indices || (!out_enc && !out_ext) || t == 0 || t > (1u << 20) || m > (size_t(1) << 28) / k) return fail(KYB_E_BAD_ARG, "bad argument");
  if (max_index == 0xffffffffu) return fail(KYB_E_BAD_ARG, "index + 1 must fit 32 bits");
  if (!aligned16(commits_ext) || !aligned16(out_enc) || !aligned16(out_ext)) return fail(KYB_E_BAD_ARG, "device buffers must be 16-byte aligned");
  return drained(launch_poly_eval(g, commits_ext, t, indices, m * k, max_index, out_enc, out_ext, pick(g, stream), k));
}
int kyb_pubpoly_eval_multi_batch(const int32_t* commits_ext, size_t t, size_t m, const uint32_t* indices, size_t k, uint8_t* out_enc, int32_t* out_ext) {
  ENTER();
  if (m == 0 || k == 0) return KYB_OK;
  if (!commits_ext || !indices || (!out_enc && !out_ext) || t == 0 || t > (1u << 20) || m > (size_t(1) << 28) / k || m > (size_t(1) << 30) / t)
    return fail(KYB_E_BAD_ARG, "bad argument");
  const size_t n = m * k;
  uint32_t mx = 0;
  for (size_t i = 0; i < n; ++i) mx = indices[i] > mx ? indices[i] : mx;
  if (mx == 0xffffffffu) return fail(KYB_E_BAD_ARG, "index + 1 must fit 32 bits");
  HostCall c(g);
  const int ic = c.in(commits_ext, 160 * t * m), ii = c.in(indices, 4 * n), ie = c.out(out_enc, 32 * n), ix = c.out(out_ext, 160 * n);
  return c.run([&](hipStream_t st) { return drained(launch_poly_eval(g, c.dev<int32_t>(ic), t, c.dev<uint32_t>(ii), n, mx, c.dev(ie), c.dev<int32_t>(ix), st, k)); });
}
int kyb_sum_batch_dev(const int32_t* pts_ext, size_t m, size_t t, uint8_t* out_enc, int32_t* out_ext, void* stream) {
  ENTER();
  if (m == 0) return KYB_OK;
  if (t == 0 || t > (size_t(1) << 24) || m > (size_t(1) << 28) / t) return fail(KYB_E_BAD_ARG, "m * t out of range");
  if (!pts_ext || (!out_enc && !out_ext)) return fail(KYB_E_BAD_ARG, "null buffer");
  if (!aligned16(pts_ext) || !aligned16(out_enc) || !aligned16(out_ext)) return fail(KYB_E_BAD_ARG, "device buffers must be 16-byte aligned");
  return drained(launch_sum(g, pts_ext, nullptr, nullptr, false, m, t, out_enc, out_ext, pick(g, stream)));
}
int kyb_sum_batch(const int32_t* pts_ext, size_t m, size_t t, uint8_t* out_enc, int32_t* out_ext) {
  ENTER();
  if (m == 0) return KYB_OK;
  if (t == 0 || t > (size_t(1) << 24) || m > (size_t(1) << 28) / t) return fail(KYB_E_BAD_ARG, "m * t out of range");
  if (!pts_ext || (!out_enc && !out_ext)) return fail(KYB_E_BAD_ARG, "null buffer");
  HostCall c(g);
  const int ip = c.in(pts_ext, 160 * m * t), ie = c.out(out_enc, 32 * m), ix = c.out(out_ext, 160 * m);
  return c.run([&](hipStream_t st) { return drained(launch_sum(g, c.dev<int32_t>(ip), nullptr, nullptr, false, m, t, c.dev(ie), c.dev<int32_t>(ix), st)); });
}
// wire-format operands: the commitments / points as the 32-byte encodings a Deal carries, unmarshalled on the GPU
int kyb_pubpoly_eval_multi_enc_batch_dev(const uint8_t* commits_enc, size_t t, size_t m, const uint32_t* indices, size_t k, uint32_t max_index,
                                         uint8_t* out_enc, int32_t* out_ext, uint8_t* ok, void* stream) {
  ENTER();
  if (m == 0 || k == 0) return KYB_OK;
  if (!commits_enc || !indices || (!out_enc && !out_ext) || t == 0 || t > (1u << 20) || m > (size_t(1) << 28) / k || m > (size_t(1) << 30) / t)
    return fail(KYB_E_BAD_ARG, "bad argument");
  if (max_index == 0xffffffffu) return fail(KYB_E_BAD_ARG, "index + 1 must fit 32 bits");
  if (!aligned16(commits_enc) || !aligned16(out_enc) || !aligned16(out_ext)) return fail(KYB_E_BAD_ARG, "device buffers must be 16-byte aligned");
  return drained(launch_poly_eval(g, nullptr, t, indices, m * k, max_index, out_enc, out_ext, pick(g, stream), k, commits_enc, ok));
}
int kyb_pubpoly_eval_multi_enc_batch(const uint8_t* commits_enc, size_t t, size_t m, const uint32_t* indices, size_t k, uint8_t* out_enc, int32_t* out_ext,
                                     uint8_t* ok) {
  ENTER();
  if (m == 0 || k == 0) return KYB_OK;
  if (!commits_enc || !indices || (!out_enc && !out_ext) || t == 0 || t > (1u << 20) || m > (size_t(1) << 28) / k || m > (size_t(1) << 30) / t)
    return fail(KYB_E_BAD_ARG, "bad argument");
  const size_t n = m * k;
  uint32_t mx = 0;
  for (size_t i = 0; i < n; ++i) mx = indices[i] > mx ? indices[i] : mx;
  if (mx == 0xffffffffu) return fail(KYB_E_BAD_ARG, "index + 1 must fit 32 bits");
  HostCall c(g);
  const int ic = c.in(commits_enc, 32 * t * m), ii = c.in(indices, 4 * n), ie = c.out(out_enc, 32 * n), ix = c.out(out_ext, 160 * n), ik = c.out(ok, t * m);
  return c.run([&](hipStream_t st) {
    return drained(launch_poly_eval(g, nullptr, t, c.dev<uint32_t>(ii), n, mx, c.dev(ie), c.dev<int32_t>(ix), st, k, c.dev(ic), c.dev(ik)));
  });
}
int kyb_sum_enc_batch_dev(const uint8_t* pts_enc, size_t m, size_t t, int item_major, uint8_t* out_enc, int32_t* out_ext, uint8_t* ok, void* stream) {
  ENTER();
  if (m == 0) return KYB_OK;
  if (t == 0 || t > (size_t(1) << 24) || m > (size_t(1) << 28) / t) return fail(KYB_E_BAD_ARG, "m * t out of range");
  if (!pts_enc || (!out_enc && !out_ext)) return fail(KYB_E_BAD_ARG, "null buffer");
  if (!aligned16(pts_enc) || !aligned16(out_enc) || !aligned16(out_ext)) return fail(KYB_E_BAD_ARG, "device buffers must be 16-byte aligned");
  return drained(launch_sum(g, nullptr, pts_enc, ok, item_major != 0, m, t, out_enc, out_ext, pick(g, stream)));
}
int kyb_sum_enc_batch(const uint8_t* pts_enc, size_t m, size_t t, int item_major, uint8_t* out_enc, int32_t* out_ext, uint8_t* ok) {
  ENTER();
  if (m == 0) return KYB_OK;
  if (t == 0 || t > (size_t(1) << 24) || m > (size_t(1) << 28) / t) return fail(KYB_E_BAD_ARG, "m * t out of range");
  if (!pts_enc || (!out_enc && !out_ext)) return fail(KYB_E_BAD_ARG, "null buffer");
  HostCall c(g);
  const int ip = c.in(pts_enc, 32 * m * t), ie = c.out(out_enc, 32 * m), ix = c.out(out_ext, 160 * m), ik = c.out(ok, m * t);
  return c.run([&](hipStream_t st) {
    return drained(launch_sum(g, nullptr, c.dev(ip), c.dev(ik), item_major != 0, m, t, c.dev(ie), c.dev<int32_t>(ix), st));
  });
}
// one verifier call per DKG round: decode the m x t commitments once, evaluate every dealer's polynomial at `index`, sum the columns
int kyb_dkg_verify_round_enc_dev(const uint8_t* commits_enc, size_t t, size_t m, const uint32_t* index_dev, uint32_t index, uint8_t* eval_enc, int32_t* eval_ext,
                                 uint8_t* sum_enc, int32_t* sum_ext, uint8_t* ok, void* stream) {
  ENTER();
  if (m == 0) return KYB_OK;
  if (!commits_enc || !index_dev || (!eval_enc && !eval_ext) || t == 0 || t > (1u << 20) || m > (size_t(1) << 28) || m > (size_t(1) << 30) / t)
    return fail(KYB_E_BAD_ARG, "bad argument");
  if (index == 0xffffffffu) return fail(KYB_E_BAD_ARG, "index + 1 must fit 32 bits");
  if (!aligned16(commits_enc) || !aligned16(eval_enc) || !aligned16(eval_ext) || !aligned16(sum_enc) || !aligned16(sum_ext))
    return fail(KYB_E_BAD_ARG, "device buffers must be 16-byte aligned");
  return drained(launch_dkg_round(g, commits_enc, t, m, index_dev, index, eval_enc, eval_ext, sum_enc, sum_ext, ok, pick(g, stream)));
}
int kyb_dkg_verify_round_enc(const uint8_t* commits_enc, size_t t, size_t m, uint32_t index, uint8_t* eval_enc, int32_t* eval_ext, uint8_t* sum_enc,
                             int32_t* sum_ext, uint8_t* ok) {
  ENTER();
  if (m == 0) return KYB_OK;
  if (!commits_enc || (!eval_enc && !eval_ext) || t == 0 || t > (1u << 20) || m > (size_t(1) << 28) || m > (size_t(1) << 30) / t) return fail(KYB_E_BAD_ARG, "bad argument");
  if (index == 0xffffffffu) return fail(KYB_E_BAD_ARG, "index + 1 must fit 32 bits");
  std::vector<uint32_t> idx(m, index);
  HostCall c(g);
  const int ic = c.in(commits_enc, 32 * t * m), ii = c.in(idx.data(), 4 * m), ie = c.out(eval_enc, 32 * m), ix = c.out(eval_ext, 160 * m),
            se = c.out(sum_enc, 32 * t), sx = c.out(sum_ext, 160 * t), ik = c.out(ok, t * m);
  return c.run([&](hipStream_t st) {
    return drained(launch_dkg_round(g, c.dev(ic), t, m, c.dev<uint32_t>(ii), index, c.dev(ie), c.dev<int32_t>(ix), c.dev(se), c.dev<int32_t>(sx), c.dev(ik), st));
  });
}
int kyb_equal_batch_dev(const int32_t* a_ext, const int32_t* b_ext, size_t n, uint8_t* eq, void* stream) {
  ENTER();
  if (n == 0) return KYB_OK;
  if (!a_ext || !b_ext || !eq) return fail(KYB_E_BAD_ARG, "null buffer");
  if (!aligned16(a_ext) || !aligned16(b_ext)) return fail(KYB_E_BAD_ARG, "device buffers must be 16-byte aligned");
  LAUNCHCK(launch::equal(pick(g, stream), a_ext, b_ext, n, eq));
  return KYB_OK;
}
int kyb_equal_batch(const int32_t* a_ext, const int32_t* b_ext, size_t n, uint8_t* eq) {
  ENTER();
  if (n == 0) return KYB_OK;
  if (!a_ext || !b_ext || !eq) return fail(KYB_E_BAD_ARG, "null buffer");
  HostCall c(g);
  const int a = c.in(a_ext, 160 * n), b = c.in(b_ext, 160 * n), e = c.out(eq, n);
  return c.run([&](hipStream_t st) { return kyb_equal_batch_dev(c.dev<int32_t>(a), c.dev<int32_t>(b), n, c.dev(e), st); });
}

int kyb_point_checks_batch_dev(const uint8_t* enc, const int32_t* pts_ext, size_t n, uint8_t* flags, void* stream) {
  ENTER();
  if (n == 0) return KYB_OK;
  if (!flags) return fail(KYB_E_BAD_ARG, "null buffer");
  if ((enc == nullptr) == (pts_ext == nullptr)) return fail(KYB_E_BAD_ARG, "give exactly one of enc / pts_ext");
  if (!aligned16(enc) || !aligned16(pts_ext)) return fail(KYB_E_BAD_ARG, "device buffers must be 16-byte aligned");
  return drained(launch_point_checks(g, enc, pts_ext, n, flags, pick(g, stream)));
}
int kyb_point_checks_batch(const uint8_t* enc, const int32_t* pts_ext, size_t n, uint8_t* flags) {
  ENTER();
  if (n == 0) return KYB_OK;
  if (!flags) return fail(KYB_E_BAD_ARG, "null buffer");
  if ((enc == nullptr) == (pts_ext == nullptr)) return fail(KYB_E_BAD_ARG, "give exactly one of enc / pts_ext");
  HostCall c(g);
  const int ie = c.in(enc, 32 * n), ix = c.in(pts_ext, 160 * n), io = c.out(flags, n);
  return c.run([&](hipStream_t st) { return drained(launch_point_checks(g, c.dev(ie), c.dev<int32_t>(ix), n, c.dev(io), st)); });
}

void* kyb_host_alloc(size_t bytes) {
  Ctx* c = cur();
  if (c == nullptr || !c->ready) { (void)fail(KYB_E_NOT_INIT, "no initialised context: kyb_init / kyb_ctx_create has not succeeded"); return nullptr; }
  (void)hipSetDevice(c->device);
  void* p = nullptr;
  const size_t want = bytes ? bytes : 1;
  hipError_t e = diag_trip(c->diag_fail_alloc) ? hipErrorOutOfMemory : hipHostMalloc(&p, want, hipHostMallocCoherent);      // coherent: results written there are read when the completion flag arrives (pinned_dev_ptr)
  if (e != hipSuccess) { (void)fail(KYB_E_NOMEM, "pinned host allocation", e); return nullptr; }
  void* dp = nullptr;
  if (hipHostGetDevicePointer(&dp, p, 0) == hipSuccess && dp != nullptr) {
    HostAllocs& h = host_allocs();
    std::lock_guard<std::mutex> lk(h.mu);
    h.recs[reinterpret_cast<uintptr_t>(p)] = HostAllocs::Rec{want, c->device, static_cast<uint8_t*>(dp) - static_cast<uint8_t*>(p)};
  } else {
    (void)hipGetLastError();                                            // not mapped: still page-locked memory for the DMA engines, never used in place
  }
  return p;
}
void kyb_host_free(void* p) {
  if (!p) return;
  { HostAllocs& h = host_allocs(); std::lock_guard<std::mutex> lk(h.mu); h.recs.erase(reinterpret_cast<uintptr_t>(p)); }
  (void)hipHostFree(p);
}

int kyb_profile_begin(int max_launches) {
  ENTER();
  if (max_launches < 0 || max_launches > 65536) return fail(KYB_E_BAD_ARG, "max_launches out of range");
  std::lock_guard<std::mutex> lk(g.prof.mu);
  for (int i = 0; i < g.prof.cap; ++i) { (void)hipEventDestroy(g.prof.recs[i].a); (void)hipEventDestroy(g.prof.recs[i].b); }
  delete[] g.prof.recs;
  g.prof.recs = nullptr; g.prof.cap = 0; g.prof.used = 0; g.prof.on = false;
  if (max_launches == 0) return KYB_OK;
  g.prof.recs = new ProfRec[max_launches];
  for (int i = 0; i < max_launches; ++i) { HIPCK(hipEventCreate(&g.prof.recs[i].a)); HIPCK(hipEventCreate(&g.prof.recs[i].b)); g.prof.cap = i + 1; }
  g.prof.on = true;
  return KYB_OK;
}
int kyb_profile_read(int* kernel_ids, float* ms, int cap, int* count) {
  ENTER();
  if (!kernel_ids || !ms || !count) return fail(KYB_E_BAD_ARG, "null argument");
  std::lock_guard<std::mutex> lk(g.prof.mu);
  g.prof.on = false;
  int nrec = g.prof.used < cap ? g.prof.used : cap;
  for (int i = 0; i < nrec; ++i) {
    HIPCK(hipEventSynchronize(g.prof.recs[i].b));
    kernel_ids[i] = g.prof.recs[i].id;
    HIPCK(hipEventElapsedTime(&ms[i], g.prof.recs[i].a, g.prof.recs[i].b));
  }
  *count = nrec;
  return KYB_OK;
}
const char* kyb_kernel_name(int kernel_id) { return (kernel_id >= 0 && kernel_id < KID_COUNT) ? KERNEL_NAMES[kernel_id] : ""; }

// options belong to the calling thread's context; they are atomics, so setting one while other threads launch is safe
// (a launch sequence already under way may still use the old value for its remaining kernels)
int kyb_set_option(const char* key, int value) {
  if (!key) return fail(KYB_E_BAD_ARG, "null key");
  ENTER();
  if (!strcmp(key, "device.cus")) {          // the compute units this context's streams really have (0 = what the device reports): thresholds and grids follow
    if (value < 0 || value > g.hw_cus) return fail(KYB_E_BAD_ARG, "device.cus in 0..the device's compute units");
    std::lock_guard<std::mutex> lk(g.mu);
    std::lock_guard<std::mutex> launch_lock(g.launch_mu);
    HIPCK(hipDeviceSynchronize());
    apply_cu_count(g, value == 0 ? g.hw_cus : value);
    return KYB_OK;
  }
  if (!strcmp(key, "coop.max_items")) { if (value < 0 || value > (1 << 20)) return fail(KYB_E_BAD_ARG, "coop.max_items in 0..2^20"); g.opt_coop_max = value; return KYB_OK; }
  if (!strcmp(key, "coop.base_max_items")) { if (value < 0 || value > (1 << 20)) return fail(KYB_E_BAD_ARG, "coop.base_max_items in 0..2^20"); g.opt_coop_base_max = value; return KYB_OK; }
  if (!strcmp(key, "coop.decode_max_items")) { if (value < 0 || value > (1 << 20)) return fail(KYB_E_BAD_ARG, "coop.decode_max_items in 0..2^20"); g.opt_coop_decode_max = value; return KYB_OK; }
  if (!strcmp(key, "host.pipe_chunks")) { if (value < 2 || value > 64) return fail(KYB_E_BAD_ARG, "host.pipe_chunks in 2..64"); g.opt_pipe_chunks = value; return KYB_OK; }
  if (!strcmp(key, "ext.projective")) { if (value != 0 && value != 1) return fail(KYB_E_BAD_ARG, "ext.projective is 0 or 1"); g.opt_ext_projective = value; return KYB_OK; }
  if (!strcmp(key, "host.in_place")) { if (value < 0 || value > 1) return fail(KYB_E_BAD_ARG, "host.in_place is 0 or 1"); g.opt_host_inplace = value; return KYB_OK; }
  if (!strcmp(key, "host.zero_copy_kib")) { if (value < 0 || value > (1 << 16)) return fail(KYB_E_BAD_ARG, "host.zero_copy_kib in 0..65536"); g.opt_zero_copy_kib = value; return KYB_OK; }
  if (!strcmp(key, "coop.share_by_load")) { if (value < 0 || value > 1) return fail(KYB_E_BAD_ARG, "coop.share_by_load in 0..1"); g.opt_coop_share = value; return KYB_OK; }
  if (!strcmp(key, "coop.ladder_max_items")) { if (value < 0) return fail(KYB_E_BAD_ARG, "coop.ladder_max_items >= 0"); g.opt_coop_ladder_max = value; return KYB_OK; }
  if (!strcmp(key, "coop.ladder_enc_max_items")) { if (value < 0) return fail(KYB_E_BAD_ARG, "coop.ladder_enc_max_items >= 0"); g.opt_coop_ladder_enc_max = value; return KYB_OK; }
  if (!strcmp(key, "ladder.quad_max_items")) { if (value < 0) return fail(KYB_E_BAD_ARG, "ladder.quad_max_items >= 0"); g.opt_ladder_quad_max = value; return KYB_OK; }
  if (!strcmp(key, "ladder.pair_max_items")) { if (value < 0) return fail(KYB_E_BAD_ARG, "ladder.pair_max_items >= 0"); g.opt_ladder_pair_max = value; return KYB_OK; }
  if (!strcmp(key, "ladder.skip_canonical")) { if (value < 0 || value > 1) return fail(KYB_E_BAD_ARG, "ladder.skip_canonical in 0..1"); g.opt_ladder_skip_canonical = value; return KYB_OK; }
  if (!strcmp(key, "mul.short_scalars")) { if (value < 0 || value > 1) return fail(KYB_E_BAD_ARG, "mul.short_scalars in 0..1"); g.opt_mul_short_scalars = value; return KYB_OK; }
  if (!strcmp(key, "coop.verify_max_items")) { if (value < 0 || value > (1 << 20)) return fail(KYB_E_BAD_ARG, "coop.verify_max_items in 0..2^20"); g.opt_coop_verify_max = value; return KYB_OK; }
  if (!strcmp(key, "host.copy_threads")) { if (value < 0 || value > 64) return fail(KYB_E_BAD_ARG, "host.copy_threads in 0..64"); g.opt_copy_threads = value; return KYB_OK; }
  if (!strcmp(key, "defer.fuse")) { if (value < 0 || value > 1) return fail(KYB_E_BAD_ARG, "defer.fuse in 0..1"); g.opt_defer_fuse = value; return KYB_OK; }
  if (!strcmp(key, "defer.max_nodes")) { if (value < 16) return fail(KYB_E_BAD_ARG, "defer.max_nodes >= 16"); g.opt_defer_max_nodes = value; return KYB_OK; }
  if (!strcmp(key, "defer.keep_mib")) { if (value < 0 || value > (1 << 20)) return fail(KYB_E_BAD_ARG, "defer.keep_mib in 0..2^20"); g.opt_defer_keep_mib = value; return KYB_OK; }
#ifdef KYB_CROSSCHECK      // kernel and algorithm VARIANTS: selectable in the cross-check build the tests compare the product against, not options of the product library
  // ... and the fault injection of tests/test_gpu_fault_injection.py
  if (!strcmp(key, "diag.fail_alloc_after")) { if (value < 0) return fail(KYB_E_BAD_ARG, "diag.fail_alloc_after >= 0"); g.diag_fail_alloc = value; return KYB_OK; }
  if (!strcmp(key, "diag.fail_launch_after")) { if (value < 0) return fail(KYB_E_BAD_ARG, "diag.fail_launch_after >= 0"); g.diag_fail_launch = value; return KYB_OK; }
  if (!strcmp(key, "mul.select")) { if (value < 0 || value > 1) return fail(KYB_E_BAD_ARG, "mul.select in {0,1}"); g.opt_mul_select = value; return KYB_OK; }
  if (!strcmp(key, "mul_base.select")) { if (value < 0 || value > 1) return fail(KYB_E_BAD_ARG, "mul_base.select in {0,1}"); g.opt_base_select = value; return KYB_OK; }
  if (!strcmp(key, "mul.algo")) { if (value < 0 || value > 1) return fail(KYB_E_BAD_ARG, "mul.algo in {0 window table, 1 ladder}"); g.opt_mul_algo = value; return KYB_OK; }
  if (!strcmp(key, "mul.ladder_waves")) { if (value < 2 || value > 4) return fail(KYB_E_BAD_ARG, "mul.ladder_waves in 2..4"); g.opt_ladder_waves = value; return KYB_OK; }
  if (!strcmp(key, "mul_base.radix")) { if (value != 16 && value != 32 && value != 64) return fail(KYB_E_BAD_ARG, "mul_base.radix in {16,32,64}"); g.opt_base_radix = value; return KYB_OK; }
  if (!strcmp(key, "mul_base.block")) { if (value != 256 && value != 512) return fail(KYB_E_BAD_ARG, "mul_base.block in {256,512}"); g.opt_base_block = value; return KYB_OK; }
  if (!strcmp(key, "finish.batched")) { if (value < 0 || value > 1) return fail(KYB_E_BAD_ARG, "finish.batched in {0,1}"); g.opt_finish = value; return KYB_OK; }
  if (!strcmp(key, "encode.batched")) { if (value < 0 || value > 1) return fail(KYB_E_BAD_ARG, "encode.batched in {0,1}"); g.opt_encode_batched = value; return KYB_OK; }
  if (!strcmp(key, "poly.batch_segments")) { if (value < 0 || value > 256) return fail(KYB_E_BAD_ARG, "poly.batch_segments in 0..256"); g.opt_poly_batch_segments = value; return KYB_OK; }
  if (!strcmp(key, "poly.segments")) { if (value < 0 || value > 32) return fail(KYB_E_BAD_ARG, "poly.segments in 0..32"); g.opt_poly_segments = value; return KYB_OK; }
  if (!strcmp(key, "verify.by_encoding")) { if (value != 0 && value != 1) return fail(KYB_E_BAD_ARG, "verify.by_encoding is 0 or 1"); g.opt_verify_by_enc = value; return KYB_OK; }
  if (!strcmp(key, "mul_base.block64")) { if (value != 512 && value != 768 && value != 1024) return fail(KYB_E_BAD_ARG, "mul_base.block64 in {512,768,1024}"); g.opt_base_block64 = value; return KYB_OK; }
  if (!strcmp(key, "mul_base.small_chunks")) { if (value < 0 || value > 64) return fail(KYB_E_BAD_ARG, "mul_base.small_chunks in 0..64"); g.opt_base_small_chunks = value; return KYB_OK; }
  if (!strcmp(key, "verify.overlap")) { g.opt_verify_overlap = value != 0; return KYB_OK; }
  if (!strcmp(key, "finish.min_items")) { if (value < 1) return fail(KYB_E_BAD_ARG, "finish.min_items >= 1"); g.opt_finish_min = value; return KYB_OK; }
  if (!strcmp(key, "ladder.y_only")) { if (value < 0 || value > 2) return fail(KYB_E_BAD_ARG, "ladder.y_only in 0..2"); g.opt_ladder_y_only = value; return KYB_OK; }
  if (!strcmp(key, "mul_base.quarters")) { if (value < 0 || value > 1) return fail(KYB_E_BAD_ARG, "mul_base.quarters in {0,1}"); g.opt_base_quarters = value; return KYB_OK; }
  if (!strcmp(key, "finish.four")) { if (value < 0 || value > 2) return fail(KYB_E_BAD_ARG, "finish.four in 0..2"); g.opt_finish_four = value; return KYB_OK; }
  if (!strcmp(key, "mul.grid_per_cu")) { if (value < 1 || value > 8) return fail(KYB_E_BAD_ARG, "mul.grid_per_cu in 1..8");
    if (value > 2) return fail(KYB_E_BAD_ARG, "workspace is sized for 2 blocks per CU");
    g.grid_mul = g.cus * value; return KYB_OK; }
#endif
  return fail(KYB_E_BAD_ARG, "unknown option");
}
int kyb_get_option(const char* key, int* value) {
  if (!key || !value) return fail(KYB_E_BAD_ARG, "null argument");
  ENTER();
  if (!strcmp(key, "defer.fuse")) { *value = g.opt_defer_fuse; return KYB_OK; }
  if (!strcmp(key, "defer.max_nodes")) { *value = g.opt_defer_max_nodes; return KYB_OK; }
  if (!strcmp(key, "defer.keep_mib")) { *value = g.opt_defer_keep_mib; return KYB_OK; }
  if (!strcmp(key, "device.cus")) { *value = g.cus; return KYB_OK; }
  if (!strcmp(key, "coop.max_items")) { *value = g.opt_coop_max; return KYB_OK; }
  if (!strcmp(key, "coop.base_max_items")) { *value = g.opt_coop_base_max; return KYB_OK; }
  if (!strcmp(key, "coop.decode_max_items")) { *value = g.opt_coop_decode_max; return KYB_OK; }
  if (!strcmp(key, "coop.verify_max_items")) { *value = g.opt_coop_verify_max; return KYB_OK; }
  if (!strcmp(key, "host.in_place")) { *value = g.opt_host_inplace; return KYB_OK; }
  if (!strcmp(key, "diag.dev_kib")) { *value = (int)(g.diag_dev_bytes.load() >> 10); return KYB_OK; }
  if (!strcmp(key, "diag.host_kib")) { *value = (int)(g.diag_host_bytes.load() >> 10); return KYB_OK; }
  if (!strcmp(key, "host.zero_copy_kib")) { *value = g.opt_zero_copy_kib; return KYB_OK; }
  if (!strcmp(key, "coop.share_by_load")) { *value = g.opt_coop_share; return KYB_OK; }
  if (!strcmp(key, "coop.ladder_max_items")) { *value = g.opt_coop_ladder_max; return KYB_OK; }
  if (!strcmp(key, "coop.ladder_enc_max_items")) { *value = g.opt_coop_ladder_enc_max; return KYB_OK; }
  if (!strcmp(key, "ladder.quad_max_items")) { *value = g.opt_ladder_quad_max; return KYB_OK; }
  if (!strcmp(key, "ladder.pair_max_items")) { *value = g.opt_ladder_pair_max; return KYB_OK; }
  if (!strcmp(key, "ladder.skip_canonical")) { *value = g.opt_ladder_skip_canonical; return KYB_OK; }
  if (!strcmp(key, "mul.short_scalars")) { *value = g.opt_mul_short_scalars; return KYB_OK; }
  if (!strcmp(key, "ext.projective")) { *value = g.opt_ext_projective; return KYB_OK; }
  if (!strcmp(key, "host.pipe_chunks")) { *value = g.opt_pipe_chunks; return KYB_OK; }
  if (!strcmp(key, "host.copy_threads")) { *value = copy_threads(g); return KYB_OK; }
#ifdef KYB_CROSSCHECK      // kernel and algorithm VARIANTS: selectable in the cross-check build the tests compare the product against, not options of the product library
  if (!strcmp(key, "diag.fail_alloc_after")) { *value = g.diag_fail_alloc; return KYB_OK; }
  if (!strcmp(key, "diag.fail_launch_after")) { *value = g.diag_fail_launch; return KYB_OK; }
  if (!strcmp(key, "mul.select")) { *value = g.opt_mul_select; return KYB_OK; }
  if (!strcmp(key, "mul_base.select")) { *value = g.opt_base_select; return KYB_OK; }
  if (!strcmp(key, "mul.algo")) { *value = g.opt_mul_algo; return KYB_OK; }
  if (!strcmp(key, "mul.ladder_waves")) { *value = g.opt_ladder_waves; return KYB_OK; }
  if (!strcmp(key, "mul_base.radix")) { *value = g.opt_base_radix; return KYB_OK; }
  if (!strcmp(key, "mul_base.block")) { *value = g.opt_base_block; return KYB_OK; }
  if (!strcmp(key, "finish.batched")) { *value = g.opt_finish; return KYB_OK; }
  if (!strcmp(key, "encode.batched")) { *value = g.opt_encode_batched; return KYB_OK; }
  if (!strcmp(key, "ladder.y_only")) { *value = g.opt_ladder_y_only; return KYB_OK; }
  if (!strcmp(key, "mul_base.quarters")) { *value = g.opt_base_quarters; return KYB_OK; }
  if (!strcmp(key, "finish.four")) { *value = g.opt_finish_four; return KYB_OK; }
  if (!strcmp(key, "verify.by_encoding")) { *value = g.opt_verify_by_enc; return KYB_OK; }
  if (!strcmp(key, "poly.batch_segments")) { *value = g.opt_poly_batch_segments; return KYB_OK; }
  if (!strcmp(key, "poly.segments")) { *value = g.opt_poly_segments; return KYB_OK; }
  if (!strcmp(key, "mul_base.block64")) { *value = g.opt_base_block64; return KYB_OK; }
  if (!strcmp(key, "mul_base.small_chunks")) { *value = g.opt_base_small_chunks; return KYB_OK; }
  if (!strcmp(key, "verify.overlap")) { *value = g.opt_verify_overlap; return KYB_OK; }
  if (!strcmp(key, "finish.min_items")) { *value = g.opt_finish_min; return KYB_OK; }
  if (!strcmp(key, "mul.grid_per_cu")) { *value = g.cus ? g.grid_mul / g.cus : 0; return KYB_OK; }
#endif
  return fail(KYB_E_BAD_ARG, "unknown option");
}

// ---- test hooks: compiled into the CROSS-CHECK build only (the tests' library); the product library exports neither ----------
#ifdef KYB_CROSSCHECK
// test hook, not part of the documented ABI: one cooperative primitive on caller-supplied quads (host pointers, 64 words each)
int kyb_diag_coop(int op, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  ENTER(); REQUIRE_TABLE();
  HostCall c(g);
  const int ia = c.in(a, 256), ib = c.in(b, 256), io = c.out(out, 256);
  return c.run([&](hipStream_t st) {
    LAUNCHCK(launch::coop_selftest(st, op, c.dev<uint32_t>(ia), c.dev<uint32_t>(ib), c.dev<uint32_t>(io), g.table_coop));
    return KYB_OK;
  });
}

// test hook, not part of the documented ABI: one field / scalar primitive per item on caller-supplied raw limbs (host pointers, 16 words per
// item in a, b, c and out, one word per item in param; op: selftest_ops.h)
int kyb_diag_fe(int op, size_t n, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* param, uint32_t* out) {
  ENTER();
  if (op < 0 || op >= (int)FE_SELFTEST_OPS) return fail(KYB_E_BAD_ARG, "unknown self-test op");
  if (n == 0) return KYB_OK;
  if (!a || !b || !c || !param || !out) return fail(KYB_E_BAD_ARG, "null argument");
  if (n > (size_t(1) << 24)) return fail(KYB_E_BAD_ARG, "too many items");
  HostCall hc(g);
  const int ia = hc.in(a, 64 * n), ib = hc.in(b, 64 * n), ic = hc.in(c, 64 * n), ip = hc.in(param, 4 * n), io = hc.out(out, 64 * n);
  return hc.run([&](hipStream_t st) {
    LAUNCHCK(launch::fe_selftest(st, (uint32_t)op, n, hc.dev<uint32_t>(ia), hc.dev<uint32_t>(ib), hc.dev<uint32_t>(ic), hc.dev<uint32_t>(ip), hc.dev<uint32_t>(io)));
    return KYB_OK;
  });
}

// phase stamps of the one-item kernels (kernels_coop.hip KYB_PHASE): dev_buf = 32 x uint64 of device memory, zeroed by the caller; NULL = off
int kyb_diag_phase_stamps(void* dev_buf) {
  ENTER();
  if (dev_buf != nullptr && (reinterpret_cast<uintptr_t>(dev_buf) & 7u) != 0) return fail(KYB_E_BAD_ARG, "stamp buffer must be 8-byte aligned");
  std::lock_guard<std::mutex> launch_lock(g.launch_mu);
  HIPCK(hipDeviceSynchronize());
  HIPCK(launch::diag_phase_stamps(static_cast<uint64_t*>(dev_buf)));
  return KYB_OK;
}

// what the context's buffers hold NOW, for the secret-hygiene tests: `which` names a buffer (include/kyber_ed25519.h), up to `cap` bytes
// of it are copied to `dst` (device buffers after the context's streams have drained), *bytes = the buffer's size
int kyb_diag_scratch_read(int which, uint8_t* dst, size_t cap, size_t* bytes) {
  ENTER();
  if (!bytes || (cap && !dst)) return fail(KYB_E_BAD_ARG, "null argument");
  std::lock_guard<std::mutex> lk(g.mu);
  std::lock_guard<std::mutex> launch_lock(g.launch_mu);
  HIPCK(hipDeviceSynchronize());
  StreamRes* own = nullptr;
  for (StreamRes* r : g.res) if (r->own && r->stream == g.stream) own = r;
  const void* src = nullptr; size_t n = 0; bool dev = false;
  switch (which) {
    case 0: case 1: src = g.pin[which]; n = g.pin_bytes[which]; break;                       // page-locked zero-copy / bounce buffers
    case 2: src = g.stage; n = g.stage_bytes; dev = true; break;                             // device staging of the host-pointer calls
    case 3: src = g.pin_out; n = g.pin_out_bytes; break;                                     // landing area of pageable results (large calls)
    case 4: if (own) { src = own->proj; n = own->proj ? proj_alloc_bytes(own->proj_items) : 0; dev = true; } break;      // per-stream scratch of the engine stream:
    case 5: if (own) { src = own->enc; n = own->enc_bytes; dev = true; } break;                                          //   projective records, encodings,
    case 6: if (own) { src = own->part; n = own->part ? own->part_items * 160 : 0; dev = true; } break;                   //   products of small linear combinations
    case 7: if (own) { src = own->pieces; n = own->pieces ? COOP_PIECES_BYTES : 0; dev = true; } break;                   //   pieces of the four-workgroup variable-base product
    default: return fail(KYB_E_BAD_ARG, "kyb_diag_scratch_read: which in 0..7");
  }
  *bytes = src ? n : 0;
  const size_t take = *bytes < cap ? *bytes : cap;
  if (take == 0) return KYB_OK;
  if (dev) HIPCK(hipMemcpy(dst, src, take, hipMemcpyDeviceToHost)); else memcpy(dst, src, take);
  return KYB_OK;
}
#endif

// ---- benchmark diagnostics (bench.py, tools/ladder_clock.py): no product call depends on them ------------------------
int kyb_diag_wave_stamps(void* dev_buf) {
  ENTER();
  if (dev_buf != nullptr && (reinterpret_cast<uintptr_t>(dev_buf) & 7u) != 0) return fail(KYB_E_BAD_ARG, "stamp buffer must be 8-byte aligned");
  std::lock_guard<std::mutex> launch_lock(g.launch_mu);          // not between two kernels of one launch sequence of this context
  HIPCK(hipDeviceSynchronize());                                 // nor under a running kernel: the slot is read at wavefront start and end
  HIPCK(launch::diag_stamps_ladder(static_cast<uint64_t*>(dev_buf)));
  HIPCK(launch::diag_stamps_base(static_cast<uint64_t*>(dev_buf)));
  g.stamps_on = dev_buf != nullptr;
  return KYB_OK;
}
int kyb_diag_mad_peak(double min_ms, double* mads_per_s, double* clock_ghz, double* simd_cycles_per_mad, double* kernel_ms) {
  ENTER();
  if (!(min_ms >= 0.0) || min_ms > 5000.0) return fail(KYB_E_BAD_ARG, "min_ms in 0..5000");
  std::lock_guard<std::mutex> lk(g.mu);
  const int grid = g.cus * 2;                        // two 1024-thread workgroups per CU: 8 wavefronts per SIMD
  const size_t waves = (size_t)grid * 16;
  uint64_t* stamps = nullptr;
  hipEvent_t ea = nullptr, eb = nullptr;
  auto cleanup = on_scope_exit([&] { if (stamps) (void)hipFree(stamps); if (ea) (void)hipEventDestroy(ea); if (eb) (void)hipEventDestroy(eb); });
  HIPCK(hipMalloc(reinterpret_cast<void**>(&stamps), 128));
  uint32_t* sink = reinterpret_cast<uint32_t*>(stamps + 8);
  HIPCK(hipEventCreate(&ea));
  HIPCK(hipEventCreate(&eb));
  int iters = 2048;
  float ms = 0.0f;
  for (int pass = 0; pass < 6; ++pass) {             // calibrate the iteration count on the VCC form
    HIPCK(hipEventRecord(ea, g.stream));
    LAUNCHCK(launch::diag_mad_peak(g.stream, grid, iters, nullptr, sink, false));
    HIPCK(hipEventRecord(eb, g.stream));
    HIPCK(hipEventSynchronize(eb));
    HIPCK(hipEventElapsedTime(&ms, ea, eb));
    if ((double)ms >= min_ms) break;
    const double scale = min_ms / ((double)ms > 0.01 ? (double)ms : 0.01) * 1.1;
    const double want = (double)iters * (scale > 1.0 ? scale : 1.0);
    iters = want > 3.0e7 ? 30000000 : (int)want;
  }
  // the measured passes: carry-out to VCC (what the product kernels write) and to an SGPR pair; the faster one is the roofline
  double best_rate = 0.0, best_ghz = 0.0, best_cyc = 0.0, best_ms = 0.0;
  const double per_wave = (double)iters * (double)(launch::MAD_PEAK_CHAINS_HOST * launch::MAD_PEAK_UNROLL_HOST);
  for (int form = 0; form < 2; ++form) {
    HIPCK(hipMemsetAsync(stamps, 0, 128, g.stream));
    HIPCK(hipEventRecord(ea, g.stream));
    LAUNCHCK(launch::diag_mad_peak(g.stream, grid, iters, stamps, sink, form == 1));
    HIPCK(hipEventRecord(eb, g.stream));
    HIPCK(hipEventSynchronize(eb));
    HIPCK(hipEventElapsedTime(&ms, ea, eb));
    uint64_t host[5];
    HIPCK(hipMemcpy(host, stamps, sizeof(host), hipMemcpyDeviceToHost));
    const double cyc = (double)(host[2] - host[0]), rt = (double)(host[3] - host[1]);
    if (host[4] != waves || !(rt > 0.0) || !(ms > 0.0f)) return fail(KYB_E_HIP, "mad-peak kernel left no stamps");
    const double ghz = cyc / rt * 0.1;               // s_memrealtime ticks at 100 MHz
    const double rate = (double)waves * 64.0 * per_wave / ((double)ms * 1e-3);
    if (rate > best_rate) {
      best_rate = rate; best_ghz = ghz; best_ms = (double)ms;
      best_cyc = (double)ms * 1e-3 * ghz * 1e9 / ((double)waves / ((double)g.cus * 4.0) * per_wave);
    }
  }
  if (mads_per_s) *mads_per_s = best_rate;
  if (clock_ghz) *clock_ghz = best_ghz;
  if (simd_cycles_per_mad) *simd_cycles_per_mad = best_cyc;
  if (kernel_ms) *kernel_ms = best_ms;
  return KYB_OK;
}

}  // extern "C"
