// Deferred evaluation behind the per-element trait (include/kyber_ed25519.h, "deferred points"; VERDICT r3 item 2).
//
// kyber-rs's protocol code calls `Point::mul` / `add` / `sub` / `neg` one element at a time (group.rs:85-140) and looks at the result much
// later — when it marshals, compares or hashes it.  A batch-of-1 engine call costs 27-190 us, two to three times what the CPU needs, and
// every speed-up of this engine needs batches.  So the calling side may hand its operations over WITHOUT asking for the result: each
// kyb_defer_* call records a node in the context's arena and returns a handle; nothing runs until somebody asks for bytes or limbs
// (kyb_defer_get / _equal / _flush).  A flush then evaluates the recorded graph with as few engine calls as it can:
//   * nodes whose operands are known are grouped by operation, one batch call per group and level (PriPoly::commit, poly.rs:195-206: t
//     independent multiplications -> ONE call);
//   * a Horner chain  v = x v + c_j  with one small multiplier x (PubPoly::eval, poly.rs:457-469: 2 t dependent calls in the reference) is
//     recognised and becomes ONE kyb_pubpoly_eval_multi_batch call — chains of equal length found in the same flush share it;
//   * a chain of additions  acc = acc + term_j  (recover_commit, poly.rs:566-603; the dealers' sums of dkg.rs:905-953) becomes one batched
//     multiplication of its terms and ONE kyb_sum_batch call;
//     (the END of a chain need not be what was asked for: DSS::process_partial_sig, dss_sig.rs:266-273, multiplies one evaluation by the
//     challenge and adds the other to the product before it compares — both evaluations are still one call: tests/cpp/test_dss_round.cpp)
//   * when bytes are asked for, everything evaluated in that flush is marshalled on the way (the kernels' shared inversions), so the
//     marshal_binary calls that follow are cache hits.
// The evaluator is host logic on top of the ordinary host-pointer entry points of this file's ABI: the bytes are those of the eager calls
// (the GROUP ELEMENT is the same; its projective representation may differ, which no encoding shows).  Scalars are kept in the arena until
// their node has been evaluated and wiped then.  Horner fusion treats the chain's common multiplier as PUBLIC (it is a share index): a
// multiplier 1 <= x < 2^32 repeated along a chain of at least two steps — a uniformly random secret has that shape with probability 2^-220;
// `defer.fuse = 0` switches every fusion off.
//
// Handles are 64 bits, never reused: the arena's process-wide number in the upper 24, a sequence number in the lower 40.  The reference's
// Point is `Copy` (and Send): copies of a handle may live anywhere, in any thread, so nodes are not reference-counted — the arena keeps
// the youngest `defer.max_nodes` nodes with their graph (the window) and, behind it, the VALUES of the nodes that were evaluated
// (struct DeferArena, "values of EVALUATED nodes"; defer.keep_mib): a handle keeps answering and keeps working as an operand long after
// the window has moved past its node.  kyb_defer_floor (the host's word that everything older than a mark is done with, e.g. at the end
// of a protocol round) drops nodes and values; using a handle that names neither is an error (KYB_E_STALE), never a wrong answer.  A handle names its arena, so a point recorded by one thread's context can be read — and used as an operand — by a thread
// with another context (the evaluation then runs on the READER's context: nodes and scalars are host memory); an arena outlives its
// context as an "orphan" (a worker thread may end while the points it returned are still only recorded), the oldest orphans are freed
// when more than sixteen exist.
// HOST COST (round 5): a node is a 40-byte header in a chunked array; the 224 bytes of scalar, limbs and bytes live in a slab and exist only for
// nodes that need them (leaves, multiplications, evaluated results — not the inner additions of a chain that is evaluated as a sum).  The analysis
// of a flush keeps its working state IN the headers, stamped with the flush's number, and takes the nodes in ascending order — operands are always
// older than their consumers, so that IS a topological order and the dependency levels fall out of one pass; no hashing anywhere on the path
// (tests/hostcheck/defer_bench.cpp: 64 x 43 additions recorded and analysed in 0.25 ms of host time, 1.1 ms before).
namespace {
enum : uint8_t { D_INPUT = 0, D_NULL, D_BASE, D_MULBASE, D_MUL, D_ADD, D_SUB, D_NEG };
enum : uint8_t { F_VAL = 1, F_ENC = 2, F_DEAD = 4 };          // F_DEAD: inside a chain that was evaluated as a whole — not evaluated unless somebody asks for this very node
enum : uint8_t { S_SEEN = 1, S_ASKED = 2, S_SKIPPED = 4, S_NEED = 8, S_TRIED = 16 };      // working state of one flush (valid while DHdr::epoch is that flush's number)
struct DPay { uint8_t sc[32]; int32_t val[40]; uint8_t enc[32]; };
struct DHdr {
  uint64_t a = 0, b = 0;                  // operands (sequence numbers in this arena)
  uint32_t pay = 0;                       // payload slot + 1; 0: none
  uint32_t epoch = 0;
  int32_t cons = 0, level = 0, plan = -1;
  uint8_t op = D_INPUT, flags = 0, scratch = 0;
};
constexpr int CHUNK_SHIFT = 12, PAY_SHIFT = 8;
constexpr uint64_t CHUNK = (uint64_t)1 << CHUNK_SHIFT;
}  // namespace
struct DeferArena {
  std::mutex mu;
  uint32_t id = 0;                        // process-wide number: bits 40..63 of every handle this arena hands out
  // nodes first_id .. next_id - 1, in chunks of 4,096 headers; chunk0_id is the sequence number of chunks[0][0]
  std::deque<std::unique_ptr<DHdr[]>> chunks;
  uint64_t chunk0_id = 0, first_id = 1, next_id = 1;
  std::vector<std::unique_ptr<DPay[]>> pay_blocks;      // 256 payloads each
  std::vector<uint32_t> pay_free;
  uint32_t pay_used = 0;
  std::vector<uint64_t> pending;          // ids recorded and not evaluated yet (may hold ids evaluated meanwhile: filtered at use)
  uint32_t epoch = 0;
  bool have_base = false;
  int32_t base[40];
  // hash of a leaf's 160 bytes -> its sequence number (open addressing): a Copy type cannot remember the handle of its own limbs, and the
  // commitments of a polynomial are operands of every evaluation (n t leaves otherwise)
  std::vector<std::pair<uint64_t, uint64_t>> seen;
  size_t seen_used = 0;
  uint64_t st_flushes = 0, st_calls = 0, st_horner = 0, st_sums = 0, st_nodes = 0, st_evicted = 0, st_enc_hits = 0;
  std::vector<uint64_t> w_list, w_stack, w_need;      // working vectors of a flush, kept for their capacity
  std::vector<uint64_t> unenc;            // evaluated without their bytes (a flush that served a projective comparison): marshalled together at the first miss
  // ---- values of EVALUATED nodes that have left the window (first_id .. next_id) ------------------------------------------------------------
  // The reference's Point is Copy: a binding's point of a recorded operation is nothing but its handle, copies of it sit in protocol state for
  // the life of a node (dkg.rs:41,170; dss_sig.rs:44) and nobody can tell the arena when the last one is gone.  So a node that HAS a value
  // takes it along when the window moves past it — 200 bytes in a table keyed by its sequence number — and its handle keeps working: asked
  // for, it answers from the table; used as an operand, it comes back into the window as a leaf.  The table is bounded by bytes
  // (defer.keep_mib); when full, the entries nobody has touched since they were last looked over go first (second-chance order), so a
  // distributed key that is marshalled every round stays while the commitments of finished rounds go.  What is NOT kept: nodes that never
  // got a value — the inner steps of a chain that was evaluated as a whole (F_DEAD); anything else still unevaluated when the window
  // reaches it is evaluated first (make_room).  Values may be shared secrets: wiped when they leave.
  struct Kept { uint64_t seq; int32_t val[40]; uint8_t enc[32]; uint8_t has_enc, used; };
  std::vector<std::unique_ptr<Kept[]>> kept_blocks;      // slab in blocks of 4,096 records that never move (a growing vector would leave unwiped copies behind)
  uint32_t kept_slots = 0;
  Kept& kept_slot(uint32_t slot) { return kept_blocks[slot >> 12][slot & 4095u]; }
  std::vector<uint32_t> kept_free;
  std::deque<uint32_t> kept_order;        // slots in the order they will be looked over
  std::unordered_map<uint64_t, uint32_t> kept_at;      // sequence number -> slot
  uint64_t st_kept_dropped = 0, st_kept_hits = 0, st_readmitted = 0;
  Kept* kept_find(uint64_t seq) {
    auto it = kept_at.find(seq);
    if (it == kept_at.end()) return nullptr;
    Kept& k = kept_slot(it->second);
    k.used = 1;
    ++st_kept_hits;
    return &k;
  }
  void kept_drop_slot(uint32_t slot) {
    kept_at.erase(kept_slot(slot).seq);
    explicit_bzero(&kept_slot(slot), sizeof(Kept));
    kept_free.push_back(slot);
    ++st_kept_dropped;
  }
  void kept_put(uint64_t seq, const DPay& p, bool has_enc, size_t max_entries) {
    if (max_entries == 0) return;
    while (kept_at.size() >= max_entries && !kept_order.empty()) {      // full: second chance for what was touched, out with the rest
      const uint32_t slot = kept_order.front(); kept_order.pop_front();
      if (kept_slot(slot).used) { kept_slot(slot).used = 0; kept_order.push_back(slot); } else kept_drop_slot(slot);
    }
    uint32_t slot;
    if (!kept_free.empty()) { slot = kept_free.back(); kept_free.pop_back(); }
    else {
      if ((kept_slots & 4095u) == 0) kept_blocks.emplace_back(new Kept[4096]());
      slot = kept_slots++;
    }
    Kept& k = kept_slot(slot);
    k.seq = seq; k.has_enc = has_enc ? 1 : 0; k.used = 0;
    memcpy(k.val, p.val, 160);
    if (has_enc) memcpy(k.enc, p.enc, 32); else memset(k.enc, 0, 32);
    kept_at[seq] = slot;
    kept_order.push_back(slot);
  }
  void kept_drop_below(uint64_t seq) {    // kyb_defer_floor: the host says nothing older than the mark is wanted any more
    for (size_t i = kept_order.size(); i-- > 0;) {
      const uint32_t slot = kept_order.front(); kept_order.pop_front();
      if (kept_slot(slot).seq < seq) kept_drop_slot(slot); else kept_order.push_back(slot);
    }
  }

  size_t size() const { return (size_t)(next_id - first_id); }
  DHdr* node(uint64_t id) {
    if (id < first_id || id >= next_id) return nullptr;
    const uint64_t o = id - chunk0_id;
    return &chunks[(size_t)(o >> CHUNK_SHIFT)][(size_t)(o & (CHUNK - 1))];
  }
  DPay* pay(const DHdr& h) { return h.pay ? &pay_blocks[(h.pay - 1) >> PAY_SHIFT][(h.pay - 1) & ((1u << PAY_SHIFT) - 1)] : nullptr; }
  DPay* pay_make(DHdr& h) {
    if (h.pay == 0) {
      if (pay_free.empty()) {
        const uint32_t base_slot = (uint32_t)pay_blocks.size() << PAY_SHIFT;
        pay_blocks.emplace_back(new DPay[1u << PAY_SHIFT]);
        for (uint32_t i = 1u << PAY_SHIFT; i-- > 0;) pay_free.push_back(base_slot + i);
      }
      h.pay = pay_free.back() + 1;
      pay_free.pop_back();
      ++pay_used;
    }
    return pay(h);
  }
  // a node that leaves the arena takes its scalar, its point (it may be a Diffie-Hellman shared secret) and the bytes with it
  // (explicit_bzero: a store in front of a free is otherwise the compiler's to drop)
  // keep_entries: room in the table of kept values (0: the node's value goes with it — kyb_defer_floor, defer.keep_mib = 0)
  void drop_front(size_t keep_entries = 0) {
    DHdr& h = *node(first_id);
    if (h.pay && (h.flags & F_VAL) && h.op != D_INPUT && keep_entries != 0) kept_put(first_id, *pay(h), (h.flags & F_ENC) != 0, keep_entries);      // (a leaf is its owner's limbs: registered again when it is next an operand)
    if (h.pay) { explicit_bzero(pay(h), sizeof(DPay)); pay_free.push_back(h.pay - 1); h.pay = 0; --pay_used; }
    ++first_id;
    while (!chunks.empty() && first_id >= chunk0_id + CHUNK && next_id >= chunk0_id + CHUNK) { chunks.pop_front(); chunk0_id += CHUNK; }
  }
  DHdr& push() {
    if (chunks.empty()) chunk0_id = next_id & ~(CHUNK - 1);
    while (next_id - chunk0_id >= chunks.size() * CHUNK) chunks.emplace_back(new DHdr[CHUNK]);
    DHdr& h = *(&chunks[(size_t)((next_id - chunk0_id) >> CHUNK_SHIFT)][(size_t)((next_id - chunk0_id) & (CHUNK - 1))]);
    h = DHdr();
    ++next_id;
    return h;
  }
  ~DeferArena() {
    for (auto& b : pay_blocks) explicit_bzero(b.get(), sizeof(DPay) << PAY_SHIFT);
    for (auto& b : kept_blocks) explicit_bzero(b.get(), sizeof(Kept) * 4096);
  }
};
namespace {
constexpr int H_SHIFT = 40;
constexpr uint64_t H_SEQ_MASK = ((uint64_t)1 << H_SHIFT) - 1;
std::mutex g_arena_mu;
std::unordered_map<uint32_t, std::shared_ptr<DeferArena>> g_arenas;      // every arena of the process, live or orphaned
std::deque<uint32_t> g_orphans;                                          // arenas whose context is gone, oldest first
uint32_t g_arena_next = 1;
}  // namespace
// the context is going away: its arena stays readable (and evaluable, by whoever asks) until sixteen younger orphans exist
void defer_release(DeferArena* a) {
  std::lock_guard<std::mutex> lk(g_arena_mu);
  g_orphans.push_back(a->id);
  while (g_orphans.size() > 16) { g_arenas.erase(g_orphans.front()); g_orphans.pop_front(); }
}
namespace {

DeferArena& arena_of(Ctx& g) {
  DeferArena* have = g.defer.load(std::memory_order_acquire);
  if (have != nullptr) return *have;
  std::lock_guard<std::mutex> lk(g.launch_mu);
  if (g.defer.load(std::memory_order_relaxed) == nullptr) {
    auto a = std::make_shared<DeferArena>();
    std::lock_guard<std::mutex> rk(g_arena_mu);
    a->id = g_arena_next++ & 0xffffffu;
    if (a->id == 0) a->id = g_arena_next++ & 0xffffffu;
    g_arenas[a->id] = a;
    g.defer.store(a.get(), std::memory_order_release);
  }
  return *g.defer.load(std::memory_order_relaxed);
}
inline uint64_t handle_of(const DeferArena& A, uint64_t seq) { return ((uint64_t)A.id << H_SHIFT) | seq; }
inline uint32_t arena_id_of(uint64_t h) { return (uint32_t)(h >> H_SHIFT); }
inline uint64_t seq_of(uint64_t h) { return h & H_SEQ_MASK; }
std::shared_ptr<DeferArena> arena_by_handle(uint64_t h) {
  std::lock_guard<std::mutex> lk(g_arena_mu);
  auto it = g_arenas.find(arena_id_of(h));
  return it == g_arenas.end() ? nullptr : it->second;
}
int dcheck(DeferArena& A, uint64_t id) {
  if (id == 0) return fail(KYB_E_BAD_ARG, "deferred point: null handle");
  if (id < A.first_id) return fail(KYB_E_STALE, "deferred point: stale handle (dropped by kyb_defer_floor, never evaluated before defer.max_nodes younger nodes existed, or pushed out of defer.keep_mib)");
  if (id >= A.next_id) return fail(KYB_E_BAD_ARG, "deferred point: unknown handle");
  return KYB_OK;
}
int dflush(Ctx& g, DeferArena& A, const uint64_t* targets, size_t nt, bool want_enc, bool eq_ask = false);
inline size_t window_cap(Ctx& g) { const int opt = g.opt_defer_max_nodes.load(std::memory_order_relaxed); return (size_t)(opt > 16 ? opt : 16); }
// (a NEGATIVE value counts entries, not MiB: kyb_set_option refuses it — the seam through which tests/hostcheck/defer_host.cpp runs its random graphs
// against a table of a few dozen values)
inline size_t keep_entries(Ctx& g) {
  const int v = g.opt_defer_keep_mib.load(std::memory_order_relaxed);
  return v < 0 ? (size_t)(-(long long)v) : ((size_t)v << 20) / sizeof(DeferArena::Kept);
}
// Room for k new nodes: the window moves on — by a quarter of its size at a time, so that the flush below comes once per quarter window, not
// once per node.  Before anything leaves, EVERYTHING still pending is evaluated (one flush; protocol code looks at its results every few
// hundred operations, so little is pending): nodes that leave then have their values, which go into the table of kept values, and nodes that
// stay no longer need the operands that leave.  The only handles that die here are the inner steps of chains that were evaluated as a whole
// (F_DEAD: no value ever), which no caller holds — PubPoly::eval's accumulator is a local that is overwritten (poly.rs:457-469).  A.mu held.
inline uint64_t evict_bound(Ctx& g, DeferArena& A, size_t k) {
  const size_t cap = window_cap(g);
  if (A.size() + k <= cap) return A.first_id;
  const size_t must = A.size() + k - cap, chunk = cap / 4;
  const uint64_t upto = A.first_id + (must > chunk ? must : chunk);
  return upto < A.next_id ? upto : A.next_id;
}
int make_room(Ctx& g, DeferArena& A, size_t k) {
  const uint64_t upto = evict_bound(g, A, k);
  if (upto == A.first_id) return KYB_OK;
  bool pending = false;
  for (uint64_t id : A.pending) { DHdr* n = A.node(id); if (n && !(n->flags & (F_VAL | F_DEAD))) { pending = true; break; } }
  if (pending) { int rc = dflush(g, A, nullptr, 0, false); if (rc) return rc; }
  // An inner step of a chain that was evaluated as a whole has no value.  While it stays in the window it can still be evaluated from its operands
  // — asked for by name, or as the operand of a node recorded later (a caller may hold it: `v = x v + c` leaves every intermediate v in a Copy
  // variable) — so it gets its value NOW if an operand of it is about to leave: the chains the window's edge cuts through, a handful per move.
  // (Found by the random graphs of tests/hostcheck/defer_host.cpp through a window of 48: without this, a node recorded on such a step could
  // never be evaluated, and every later flush failed with it.)
  {
    std::vector<uint64_t> cut;
    for (uint64_t id = upto; id < A.next_id; ++id) {
      DHdr* n = A.node(id);
      if ((n->flags & (F_VAL | F_DEAD)) != F_DEAD) continue;
      const bool one = n->op == D_MUL || n->op == D_NEG, two = n->op == D_ADD || n->op == D_SUB;
      if (((one || two) && n->a < upto) || (two && n->b < upto)) cut.push_back(id);
    }
    if (!cut.empty()) { int rc = dflush(g, A, cut.data(), cut.size(), false); if (rc) return rc; }
  }
  const size_t keep = keep_entries(g);
  while (A.first_id < upto) { A.drop_front(keep); ++A.st_evicted; }
  return KYB_OK;
}
// (the caller has made room: make_room)
DHdr& dnew(DeferArena& A, uint8_t op, uint64_t a, uint64_t b, const uint8_t* sc, uint64_t* id_out) {
  *id_out = A.next_id;
  DHdr& h = A.push();
  h.op = op; h.a = a; h.b = b;
  if (sc) memcpy(A.pay_make(h)->sc, sc, 32);
  ++A.st_nodes;
  return h;
}
// are two multipliers the same 32 bytes?  All bytes are looked at whatever they hold: the operands may be secrets (then the answer is "no" and nothing
// else about them is learnt; a chain is only taken for a Horner evaluation when consecutive multipliers are EQUAL and small, which secrets are not)
inline bool sc_same(const uint8_t a[32], const uint8_t b[32]) {
  uint64_t x[4], y[4];
  memcpy(x, a, 32); memcpy(y, b, 32);
  return ((x[0] ^ y[0]) | (x[1] ^ y[1]) | (x[2] ^ y[2]) | (x[3] ^ y[3])) == 0;
}
inline bool sc_small(const uint8_t sc[32], uint32_t* index) {      // 1 <= x < 2^32: x - 1 is a share index the evaluation kernels take (0 .. 2^32 - 2)
  uint32_t high = 0;
  for (int i = 4; i < 32; ++i) high |= sc[i];
  const uint64_t x = (uint64_t)sc[0] | ((uint64_t)sc[1] << 8) | ((uint64_t)sc[2] << 16) | ((uint64_t)sc[3] << 24);
  if (high != 0 || x == 0) return false;
  *index = (uint32_t)(x - 1);
  return true;
}

// the evaluator's staging arrays carry what the nodes carry — points that may be Diffie-Hellman shared secrets, their encodings, secret multipliers:
// like the nodes' payloads they are cleared before their memory goes back to the allocator
template <class T>
struct wiped_vec : std::vector<T> {
  using std::vector<T>::vector;
  ~wiped_vec() { if (!this->empty()) explicit_bzero(this->data(), this->size() * sizeof(T)); }
};
constexpr size_t DEFER_RIDE_MAX = 64;      // fixed-base items ride in a variable-base call when both together are at most this many
struct DPlan { int kind; uint64_t sink; std::vector<uint64_t> leaves; uint32_t index; };      // kind 0: Horner (leaves = c_0 .. c_{t-1}), 1: sum of leaves

// Evaluate EVERYTHING recorded so far (whoever asks for one result will ask for the others: a dealer marshals all its commitments), and the
// `targets` (nt of them) in any case — also one that sits inside a chain an earlier flush evaluated as a whole.  want_enc: the encodings too.
// eq_ask: the flush serves Point::eq (kyb_defer_equal).  Normally it asks for the encodings too (the kernels marshal on the way; the comparison is
// then 32 bytes against 32 bytes and the marshal_binary that often follows is a hit).  But when an operand of the comparison comes out of a plain
// addition (schnorr::verify's R + h A, DSS's rand_share + hash * long_share) its bytes would cost a call of their own with an inversion of its
// own: then NOTHING of the flush is marshalled, every kernel hands over projective limbs (no inversion: 27 us less per call of few items) and the
// comparison is the projective one.
int dflush(Ctx& g, DeferArena& A, const uint64_t* targets, size_t nt, bool want_enc, bool eq_ask) {
  ++A.st_flushes;
  if (++A.epoch == 0) { for (uint64_t id = A.first_id; id < A.next_id; ++id) A.node(id)->epoch = 0; A.epoch = 1; }
  const uint32_t ep = A.epoch;
  // the working state of THIS flush in a header: valid once the header carries the flush's number
  auto touch = [&](DHdr& h) -> DHdr& { if (h.epoch != ep) { h.epoch = ep; h.cons = 0; h.level = 0; h.plan = -1; h.scratch = 0; } return h; };
  // ---- 1. the unevaluated nodes needed -------------------------------------------------------------------------------
  std::vector<uint64_t>& list = A.w_list;      // every unevaluated node reachable from the roots
  std::vector<uint64_t>& stack = A.w_stack;
  list.clear(); stack.assign(targets, targets + nt);
  {
    size_t keep = 0;
    for (uint64_t id : A.pending) { DHdr* n = A.node(id); if (n && !(n->flags & (F_VAL | F_DEAD))) { stack.push_back(id); A.pending[keep++] = id; } }
    A.pending.resize(keep);
  }
  for (size_t i = 0; i < nt; ++i) { DHdr* n = A.node(targets[i]); if (n && !(n->flags & F_VAL)) touch(*n).scratch |= S_ASKED; }
  while (!stack.empty()) {
    const uint64_t id = stack.back(); stack.pop_back();
    DHdr* n = A.node(id);
    if (!n) {      // behind the window: fine when its value was kept (an inner step of a fused chain asked for by name long after its operands left)
      if (id < A.first_id && A.kept_find(id) != nullptr) continue;
      return fail(KYB_E_STALE, "deferred point: an operand of this point left the arena without a value (stale handle)");
    }
    if (n->flags & F_VAL) continue;
    if (touch(*n).scratch & S_SEEN) continue;
    n->scratch |= S_SEEN;
    list.push_back(id);
    if (n->op == D_MUL || n->op == D_NEG) stack.push_back(n->a);
    if (n->op == D_ADD || n->op == D_SUB) { stack.push_back(n->a); stack.push_back(n->b); }
  }
  if (list.empty()) return KYB_OK;
  auto pend = [&](uint64_t id) -> DHdr* { DHdr* n = A.node(id); return n && n->epoch == ep && (n->scratch & S_SEEN) ? n : nullptr; };      // needed and unevaluated
  for (uint64_t id : list) {
    DHdr* n = A.node(id);
    auto bump = [&](uint64_t o) { if (DHdr* m = pend(o)) ++m->cons; };
    if (n->op == D_MUL || n->op == D_NEG) bump(n->a);
    if (n->op == D_ADD || n->op == D_SUB) { bump(n->a); bump(n->b); }
  }
  std::sort(list.begin(), list.end());
  // ---- 2. fusion plans ---------------------------------------------------------------------------------------------------
  // A chain's TOP may be any addition — a result somebody asked for, a sink, or a node with consumers of its own (DSS::process_partial_sig,
  // dss_sig.rs:266-270: long_poly.eval(i) goes into a multiplication, random_poly.eval(i) into an addition) — its INNER nodes have exactly one
  // consumer, the chain, and were not asked for by name.  Nodes are taken newest first: operands are older than their consumers, so the top of a
  // maximal chain is met before its inner nodes, which are marked and never tried as tops themselves.  Horner chains first, then sums over what
  // is left (a Horner result is a leaf of a sum, never an inner node of one).
  std::vector<DPlan> plans;
  if (g.opt_defer_fuse != 0) {
    // Horner: cur = ADD(MUL(x, next), c) with the same x all the way down
    for (size_t k = list.size(); k-- > 0;) {
      const uint64_t s = list[k];
      DHdr* top = A.node(s);
      if (top->op != D_ADD || (top->scratch & (S_SKIPPED | S_TRIED))) continue;
      std::vector<uint64_t> coeffs, inner;
      const uint8_t* x = nullptr;
      uint64_t cur = s, start = 0;
      for (;;) {
        DHdr* c = pend(cur);
        DHdr *ma = pend(c->a), *mb = pend(c->b);
        // (a product somebody asked for BY NAME is not chain-internal: it ends the chain, exactly as an asked-for addition does below)
        auto is_step = [&](DHdr* m) { return m && m->op == D_MUL && m->cons == 1 && !(m->scratch & S_ASKED) && (x == nullptr || sc_same(A.pay(*m)->sc, x)); };
        uint64_t mid, coef;
        if (is_step(ma)) { mid = c->a; coef = c->b; } else if (is_step(mb)) { mid = c->b; coef = c->a; }
        else { start = cur != s ? cur : 0; break; }          // the chain ends here: this addition is its leading coefficient, evaluated on its own
        DHdr* m = pend(mid);
        x = A.pay(*m)->sc;
        coeffs.push_back(coef);
        inner.push_back(mid);
        if (cur != s) inner.push_back(cur);
        DHdr* nx = pend(m->a);
        if (nx && nx->op == D_ADD && nx->cons == 1 && !(nx->scratch & S_ASKED)) { cur = m->a; continue; }
        start = m->a;
        break;
      }
      uint32_t index = 0;
      if (coeffs.size() >= 2 && start != 0 && x != nullptr && sc_small(x, &index)) {
        DHdr* st = A.node(start);
        if (!(st && st->op == D_NULL)) coeffs.push_back(start);          // x^t * start: one more coefficient (D_NULL contributes nothing)
        top->plan = (int32_t)plans.size();
        plans.push_back(DPlan{0, s, std::move(coeffs), index});
        for (uint64_t id : inner) { DHdr* h = A.node(id); h->scratch |= S_SKIPPED; h->flags |= F_DEAD; }
        ++A.st_horner;
      } else {
        // not a chain (too short, or its multiplier is no share index): neither is any tail of it — the same multiplier, fewer steps
        for (uint64_t id : inner) A.node(id)->scratch |= S_TRIED;
      }
    }
    // a chain of additions: cur = ADD(acc, term), acc again such an ADD with no other consumer
    for (size_t k = list.size(); k-- > 0;) {
      const uint64_t s = list[k];
      DHdr* top = A.node(s);
      if (top->op != D_ADD || top->plan >= 0 || (top->scratch & S_SKIPPED)) continue;
      std::vector<uint64_t> terms, inner;
      uint64_t cur = s;
      auto is_acc = [&](DHdr* m) { return m && m->op == D_ADD && m->cons == 1 && m->plan < 0 && !(m->scratch & (S_ASKED | S_SKIPPED)); };
      for (;;) {
        DHdr* c = pend(cur);
        DHdr *aa = pend(c->a), *ab = pend(c->b);
        if (is_acc(aa)) { terms.push_back(c->b); inner.push_back(c->a); cur = c->a; continue; }
        if (is_acc(ab)) { terms.push_back(c->a); inner.push_back(c->b); cur = c->b; continue; }
        terms.push_back(c->a); terms.push_back(c->b);
        break;
      }
      if (terms.size() >= 3) {
        top->plan = (int32_t)plans.size();
        plans.push_back(DPlan{1, s, std::move(terms), 0});
        for (uint64_t id : inner) { DHdr* h = A.node(id); h->scratch |= S_SKIPPED; h->flags |= F_DEAD; }
        ++A.st_sums;
      }
    }
  }
  bool projective = false;
  if (eq_ask)
    for (size_t i = 0; i < nt; ++i) {
      DHdr* n = pend(targets[i]);
      if (n && n->plan < 0 && (n->op == D_ADD || n->op == D_SUB || n->op == D_NEG)) projective = true;
    }
  if (projective) want_enc = false;
  struct ProjectiveCalls { bool on; explicit ProjectiveCalls(bool o) : on(o) { if (on) defer_projective(true); } ~ProjectiveCalls() { if (on) defer_projective(false); } } projective_calls(projective);
  // the nodes still to evaluate one by one: reachable from the roots when a planned sink is entered through its leaves
  std::vector<uint64_t>& need = A.w_need;
  need.clear(); stack.clear();
  for (uint64_t id : list) if (!(A.node(id)->scratch & S_SKIPPED)) stack.push_back(id);
  while (!stack.empty()) {
    const uint64_t id = stack.back(); stack.pop_back();
    DHdr* n = A.node(id);
    if (!n) {
      if (id < A.first_id && A.kept_find(id) != nullptr) continue;
      return fail(KYB_E_STALE, "deferred point: an operand of this point left the arena without a value (stale handle)");
    }
    if ((n->flags & F_VAL) || (touch(*n).scratch & S_NEED)) continue;
    n->scratch |= S_NEED;
    need.push_back(id);
    if (n->plan >= 0) { for (uint64_t l : plans[(size_t)n->plan].leaves) stack.push_back(l); continue; }
    if (n->op == D_MUL || n->op == D_NEG) stack.push_back(n->a);
    if (n->op == D_ADD || n->op == D_SUB) { stack.push_back(n->a); stack.push_back(n->b); }
  }
  // ---- 3. levels: operands are older than their consumers, so ascending sequence numbers are a topological order ------
  std::sort(need.begin(), need.end());
  int32_t levels = 0;
  for (uint64_t id : need) {
    DHdr* n = A.node(id);
    int32_t lv = 0;
    auto dep = [&](uint64_t o) { DHdr* m = A.node(o); if (m && !(m->flags & F_VAL) && m->epoch == ep && m->level > lv) lv = m->level; };
    if (n->plan >= 0) { for (uint64_t l : plans[(size_t)n->plan].leaves) dep(l); }
    else {
      if (n->op == D_MUL || n->op == D_NEG) dep(n->a);
      if (n->op == D_ADD || n->op == D_SUB) { dep(n->a); dep(n->b); }
      if (n->op == D_INPUT) return fail(KYB_E_BAD_ARG, "deferred point: an input node without a value");
    }
    n->level = lv + 1;
    if (n->level > levels) levels = n->level;
  }
  // A fixed-base multiplication that nothing in this flush waits for may run at any level: it is moved next to the first batch of variable-base
  // multiplications and rides in that call (below) — schnorr::verify's s B beside h A, DSS's partial B beside hash * long_share.
  {
    int32_t first_mul = 0;
    for (uint64_t id : need) { DHdr* n = A.node(id); if (n->op == D_MUL && n->plan < 0 && (first_mul == 0 || n->level < first_mul)) first_mul = n->level; }
    if (first_mul > 1)
      for (uint64_t id : need) { DHdr* n = A.node(id); if (n->op == D_MULBASE && n->cons == 0 && n->level < first_mul) n->level = first_mul; }
  }
  std::stable_sort(need.begin(), need.end(), [&](uint64_t p, uint64_t q) { return A.node(p)->level < A.node(q)->level; });
  // ---- 4. level by level: everything whose operands are known, one engine call per kind -------------------------------
  std::vector<uint64_t> done_now;
  done_now.reserve(need.size());
  // an operand's limbs: its node's, or — the window has moved past it — the kept value (checked by `known` first)
  auto val_of = [&](uint64_t id) -> const int32_t* { DHdr* n = A.node(id); return n ? A.pay(*n)->val : A.kept_find(id)->val; };
  auto call = [&](int rc) { ++A.st_calls; return rc; };
  // 1 * B as the eager calls hand it out (affine, whatever form this flush asks of its kernels): what base() nodes and riding fixed-base items use
  auto base_point = [&]() {
    uint8_t one[32] = {1};
    if (projective) defer_projective(false);
    const int rc = call(kyb_mul_base_batch(one, 1, nullptr, A.base));
    if (projective) defer_projective(true);
    if (rc == KYB_OK) A.have_base = true;
    return rc;
  };
  auto store = [&](const std::vector<uint64_t>& ids, const wiped_vec<int32_t>& ext, const wiped_vec<uint8_t>* enc) {
    for (size_t i = 0; i < ids.size(); ++i) {
      DHdr* n = A.node(ids[i]);
      DPay* p = A.pay_make(*n);
      memcpy(p->val, &ext[40 * i], 160);
      n->flags = (uint8_t)((n->flags | F_VAL) & ~F_DEAD);
      if (enc) { memcpy(p->enc, &(*enc)[32 * i], 32); n->flags |= F_ENC; }
      else if (!want_enc && A.unenc.size() < 65536) A.unenc.push_back(ids[i]);
      explicit_bzero(p->sc, 32);                        // a secret multiplier has done its work
      done_now.push_back(ids[i]);
    }
  };
  std::vector<uint64_t> r_base, r_mul, r_add, r_sub, r_host;
  std::vector<size_t> r_plan;
  for (size_t lo = 0; lo < need.size();) {
    const int32_t lv = A.node(need[lo])->level;
    size_t hi = lo;
    r_base.clear(); r_mul.clear(); r_add.clear(); r_sub.clear(); r_host.clear(); r_plan.clear();
    for (; hi < need.size() && A.node(need[hi])->level == lv; ++hi) {
      const uint64_t id = need[hi];
      DHdr* n = A.node(id);
      if (n->plan >= 0) { r_plan.push_back((size_t)n->plan); continue; }
      switch (n->op) {
        case D_NULL: case D_BASE: case D_NEG: r_host.push_back(id); break;
        case D_MULBASE: r_base.push_back(id); break;
        case D_MUL: r_mul.push_back(id); break;
        case D_ADD: r_add.push_back(id); break;
        case D_SUB: r_sub.push_back(id); break;
        default: return fail(KYB_E_BAD_ARG, "deferred point: an input node without a value");
      }
    }
    lo = hi;
    auto known = [&](uint64_t id) { DHdr* n = A.node(id); return n ? (n->flags & F_VAL) != 0 : (id < A.first_id && A.kept_find(id) != nullptr); };
    for (uint64_t id : r_mul) if (!known(A.node(id)->a)) return fail(KYB_E_BAD_ARG, "deferred point: a needed operand has left the arena without leaving a value (an engine defect: the window only moves past evaluated or never-needed nodes)");
    for (uint64_t id : r_host) {
      DHdr* n = A.node(id);
      DPay* p = A.pay_make(*n);
      if (n->op == D_NULL) { memset(p->val, 0, 160); p->val[10] = 1; p->val[20] = 1; }
      else if (n->op == D_BASE) {
        if (!A.have_base) { int rc = base_point(); if (rc) return rc; }
        memcpy(p->val, A.base, 160);
      } else {                                           // D_NEG: (-X : Y : Z : -T), limb by limb (point.rs:201-204)
        if (!known(n->a)) return fail(KYB_E_BAD_ARG, "deferred point: a needed operand has left the arena without leaving a value (an engine defect: the window only moves past evaluated or never-needed nodes)");
        const int32_t* a = val_of(n->a);
        for (int i = 0; i < 10; ++i) { p->val[i] = -a[i]; p->val[10 + i] = a[10 + i]; p->val[20 + i] = a[20 + i]; p->val[30 + i] = -a[30 + i]; }
      }
      n->flags = (uint8_t)((n->flags | F_VAL) & ~F_DEAD);
      done_now.push_back(id);
    }
    // a few fixed-base items beside a few variable-base ones: one call instead of two — s B is s * (the point B) through the variable-base
    // kernel, the same point for every scalar (both routines drop the same top digit, ge.rs:440-441, 508-568; tests pin B-as-operand against
    // the fixed-base path), and at these sizes every item has a wavefront of its own, so the call is no longer for the extra items
    if (!r_base.empty() && !r_mul.empty() && r_base.size() + r_mul.size() <= DEFER_RIDE_MAX) {
      if (!A.have_base) { int rc = base_point(); if (rc) return rc; }
      const size_t nm = r_mul.size(), n = nm + r_base.size();
      wiped_vec<uint8_t> sc(32 * n), enc(want_enc ? 32 * n : 0);
      wiped_vec<int32_t> in(40 * n), ext(40 * n);
      for (size_t i = 0; i < nm; ++i) { DHdr* d = A.node(r_mul[i]); memcpy(&sc[32 * i], A.pay(*d)->sc, 32); memcpy(&in[40 * i], val_of(d->a), 160); }
      for (size_t i = nm; i < n; ++i) { memcpy(&sc[32 * i], A.pay(*A.node(r_base[i - nm]))->sc, 32); memcpy(&in[40 * i], A.base, 160); }
      int rc = call(kyb_mul_batch(sc.data(), nullptr, in.data(), n, want_enc ? enc.data() : nullptr, ext.data(), nullptr));
      explicit_bzero(sc.data(), sc.size());
      if (rc) return rc;
      std::vector<uint64_t> ids(r_mul);
      ids.insert(ids.end(), r_base.begin(), r_base.end());
      store(ids, ext, want_enc ? &enc : nullptr);
      r_base.clear(); r_mul.clear();
    }
    if (!r_base.empty()) {
      const size_t n = r_base.size();
      wiped_vec<uint8_t> sc(32 * n), enc(want_enc ? 32 * n : 0);
      wiped_vec<int32_t> ext(40 * n);
      for (size_t i = 0; i < n; ++i) memcpy(&sc[32 * i], A.pay(*A.node(r_base[i]))->sc, 32);
      int rc = call(kyb_mul_base_batch(sc.data(), n, want_enc ? enc.data() : nullptr, ext.data()));
      explicit_bzero(sc.data(), sc.size());
      if (rc) return rc;
      store(r_base, ext, want_enc ? &enc : nullptr);
    }
    if (!r_mul.empty()) {
      const size_t n = r_mul.size();
      wiped_vec<uint8_t> sc(32 * n), enc(want_enc ? 32 * n : 0);
      wiped_vec<int32_t> in(40 * n), ext(40 * n);
      for (size_t i = 0; i < n; ++i) { DHdr* d = A.node(r_mul[i]); memcpy(&sc[32 * i], A.pay(*d)->sc, 32); memcpy(&in[40 * i], val_of(d->a), 160); }
      int rc = call(kyb_mul_batch(sc.data(), nullptr, in.data(), n, want_enc ? enc.data() : nullptr, ext.data(), nullptr));
      explicit_bzero(sc.data(), sc.size());
      if (rc) return rc;
      store(r_mul, ext, want_enc ? &enc : nullptr);
    }
    for (int sub = 0; sub < 2; ++sub) {
      const std::vector<uint64_t>& ids = sub ? r_sub : r_add;
      if (ids.empty()) continue;
      const size_t n = ids.size();
      wiped_vec<int32_t> a(40 * n), b(40 * n), ext(40 * n);
      for (size_t i = 0; i < n; ++i) {
        DHdr* d = A.node(ids[i]);
        if (!known(d->a) || !known(d->b)) return fail(KYB_E_BAD_ARG, "deferred point: a needed operand has left the arena without leaving a value (an engine defect: the window only moves past evaluated or never-needed nodes)");
        memcpy(&a[40 * i], val_of(d->a), 160); memcpy(&b[40 * i], val_of(d->b), 160);
      }
      int rc = call(kyb_add_batch(a.data(), b.data(), n, ext.data(), sub));
      if (rc) return rc;
      store(ids, ext, nullptr);
    }
    // plans of the same shape share a call
    for (int kind = 0; kind < 2; ++kind) {
      std::map<size_t, std::vector<size_t>> by_t;
      for (size_t p : r_plan) if (plans[p].kind == kind) by_t[plans[p].leaves.size()].push_back(p);
      for (auto& kv : by_t) {
        const size_t t = kv.first, m = kv.second.size();
        wiped_vec<int32_t> pts(40 * t * m), ext(40 * m);
        wiped_vec<uint8_t> enc(want_enc ? 32 * m : 0);
        std::vector<uint32_t> idx(m);
        std::vector<uint64_t> ids(m);
        for (size_t gi = 0; gi < m; ++gi) {
          const DPlan& P = plans[kv.second[gi]];
          for (size_t j = 0; j < t; ++j) {
            if (!known(P.leaves[j])) return fail(KYB_E_BAD_ARG, "deferred point: a needed operand has left the arena without leaving a value (an engine defect: the window only moves past evaluated or never-needed nodes)");
            memcpy(&pts[40 * (gi * t + j)], val_of(P.leaves[j]), 160);
          }
          idx[gi] = P.index; ids[gi] = P.sink;
        }
        int rc = kind == 0 ? call(kyb_pubpoly_eval_multi_batch(pts.data(), t, m, idx.data(), 1, want_enc ? enc.data() : nullptr, ext.data()))
                           : call(kyb_sum_batch(pts.data(), m, t, want_enc ? enc.data() : nullptr, ext.data()));
        if (rc) return rc;
        store(ids, ext, want_enc ? &enc : nullptr);
      }
    }
  }
  // ---- 5. bytes for what this flush evaluated and the kernels did not marshal on the way ------------------------------
  if (want_enc) {
    std::vector<uint64_t> ids;
    for (uint64_t id : done_now) { DHdr* n = A.node(id); if (!(n->flags & F_ENC) && n->op != D_NULL && n->op != D_BASE) ids.push_back(id); }      // constants are operands, hardly ever marshalled
    if (!ids.empty()) {
      wiped_vec<int32_t> ext(40 * ids.size());
      wiped_vec<uint8_t> enc(32 * ids.size());
      for (size_t i = 0; i < ids.size(); ++i) memcpy(&ext[40 * i], val_of(ids[i]), 160);
      int rc = call(kyb_encode_batch(ext.data(), ids.size(), enc.data()));
      if (rc) return rc;
      for (size_t i = 0; i < ids.size(); ++i) { DHdr* n = A.node(ids[i]); memcpy(A.pay(*n)->enc, &enc[32 * i], 32); n->flags |= F_ENC; }
    }
  }
  return KYB_OK;
}

// limbs (and bytes) of the point a handle names, whichever arena holds it, evaluated first if need be — on the calling thread's context
int dvalue(Ctx& g, uint64_t h, int32_t* out_ext, uint8_t* out_enc) {
  if (h == 0) return fail(KYB_E_BAD_ARG, "deferred point: null handle");
  std::shared_ptr<DeferArena> keep;
  DeferArena* own = g.defer.load(std::memory_order_acquire);
  if (own == nullptr || own->id != arena_id_of(h)) {
    keep = arena_by_handle(h);
    if (!keep) return fail(KYB_E_BAD_ARG, "deferred point: the arena that held this point is gone (its context was released long ago)");
    own = keep.get();
  }
  DeferArena& A = *own;
  std::lock_guard<std::mutex> lk(A.mu);
  const uint64_t p = seq_of(h);
  if (p != 0 && p < A.first_id) {                            // the window has moved past it: its value, if it ever had one, is in the table
    DeferArena::Kept* k = A.kept_find(p);
    if (!k) return dcheck(A, p);
    if (out_ext) memcpy(out_ext, k->val, 160);
    if (out_enc) {
      if (k->has_enc) ++A.st_enc_hits;
      else { ++A.st_calls; int rc = kyb_encode_batch(k->val, 1, k->enc); if (rc) return rc; k->has_enc = 1; }
      memcpy(out_enc, k->enc, 32);
    }
    return KYB_OK;
  }
  int rc = dcheck(A, p);
  if (rc) return rc;
  if (!(A.node(p)->flags & F_VAL)) { rc = dflush(g, A, &p, 1, out_enc != nullptr); if (rc) return rc; }
  DHdr* n = A.node(p);
  if (!n) return fail(KYB_E_BAD_ARG, "deferred point: left the arena while it was evaluated (an engine defect, never a result)");
  if (!(n->flags & F_VAL)) return fail(KYB_E_BAD_ARG, "deferred point: the evaluation finished without a value for this handle (an engine defect, never a result)");
  DPay* pay = A.pay(*n);
  if (out_ext) memcpy(out_ext, pay->val, 160);
  if (out_enc) {
    if (n->flags & F_ENC) ++A.st_enc_hits;
    else {
      // No bytes yet: the flush that evaluated it served a comparison and marshalled nothing (projective limbs: no inversion).  Whoever marshals
      // one result of such a flush marshals the others next (a dealer's commitments): all of them now, with the shared inversions of one call.
      std::vector<uint64_t> ids{p};
      for (uint64_t id : A.unenc) { DHdr* m = A.node(id); if (id != p && m && (m->flags & F_VAL) && !(m->flags & F_ENC) && m->pay) ids.push_back(id); }
      A.unenc.clear();
      wiped_vec<int32_t> ext(40 * ids.size());
      wiped_vec<uint8_t> enc(32 * ids.size());
      for (size_t i = 0; i < ids.size(); ++i) memcpy(&ext[40 * i], A.pay(*A.node(ids[i]))->val, 160);
      ++A.st_calls;
      rc = kyb_encode_batch(ext.data(), ids.size(), enc.data());
      if (rc) return rc;
      for (size_t i = 0; i < ids.size(); ++i) { DHdr* m = A.node(ids[i]); memcpy(A.pay(*m)->enc, &enc[32 * i], 32); m->flags |= F_ENC; }
    }
    memcpy(out_enc, pay->enc, 32);
  }
  return KYB_OK;
}
// enc (may be null): the 32 bytes marshal_binary yields for this point, when its owner knows them (a point unmarshalled from its canonical encoding):
// the leaf then has its bytes from the start and a comparison with an evaluated point is 32 bytes against 32 bytes, no engine call
int dinput(Ctx& g, DeferArena& A, const int32_t* ext, uint64_t* seq_out, const uint8_t* enc = nullptr) {      // A.mu held
  uint64_t w[20], h = 0x9e3779b97f4a7c15ull;               // a multiply-rotate hash over the 160 bytes; a hit is confirmed by comparing them
  memcpy(w, ext, 160);
  for (int i = 0; i < 20; ++i) { h = (h ^ w[i]) * 0xff51afd7ed558ccdull; h ^= h >> 29; }
  if (h == 0) h = 1;
  if (A.seen.empty()) A.seen.assign(1024, {0, 0});
  size_t mask = A.seen.size() - 1, at = (size_t)h & mask;
  for (; A.seen[at].first != 0; at = (at + 1) & mask) {
    if (A.seen[at].first != h) continue;
    DHdr* old = A.node(A.seen[at].second);
    if (old && old->op == D_INPUT && old->pay && memcmp(A.pay(*old)->val, ext, 160) == 0) {
      if (enc && !(old->flags & F_ENC)) { memcpy(A.pay(*old)->enc, enc, 32); old->flags |= F_ENC; }
      *seq_out = A.seen[at].second;
      return KYB_OK;
    }
  }
  if (2 * (A.seen_used + 1) > A.seen.size()) {             // half full: double, or start over beyond 2^17 leaves (old ones are mostly dropped nodes by then)
    std::vector<std::pair<uint64_t, uint64_t>> old;
    old.swap(A.seen);
    const bool restart = old.size() >= ((size_t)1 << 18);
    A.seen.assign(restart ? 1024 : 2 * old.size(), {0, 0});
    A.seen_used = 0;
    mask = A.seen.size() - 1;
    if (!restart)
      for (auto& e : old) {
        if (e.first == 0 || A.node(e.second) == nullptr) continue;
        size_t k = (size_t)e.first & mask;
        while (A.seen[k].first != 0) k = (k + 1) & mask;
        A.seen[k] = e; ++A.seen_used;
      }
    at = (size_t)h & mask;
    while (A.seen[at].first != 0) at = (at + 1) & mask;
  }
  { int rc = make_room(g, A, 1); if (rc) return rc; }
  uint64_t id = 0;
  DHdr& n = dnew(A, D_INPUT, 0, 0, nullptr, &id);
  memcpy(A.pay_make(n)->val, ext, 160);
  n.flags |= F_VAL;
  if (enc) { memcpy(A.pay(n)->enc, enc, 32); n.flags |= F_ENC; }
  A.seen[at] = {h, id}; ++A.seen_used;
  *seq_out = id;
  return KYB_OK;
}
int drecord(uint8_t op, uint64_t ha, uint64_t hb, const uint8_t* sc, uint64_t* out) {
  ENTER_HOST();
  if (!out) return fail(KYB_E_BAD_ARG, "null handle pointer");
  DeferArena& A = arena_of(g);
  const uint64_t hs[2] = {ha, hb};
  uint64_t opnd[2] = {0, 0};
  const int nop = (op == D_MUL || op == D_NEG) ? 1 : (op == D_ADD || op == D_SUB) ? 2 : 0;
  // An operand that cannot be named by a sequence number of this window comes in as a LEAF with its value: a point recorded through another
  // context (its value fetched from that arena, evaluated there if need be — before this arena's lock is taken), an operand the window has
  // moved past (from the table of kept values) or will move past when room is made for this node (from its node, evaluated now if it has to
  // be; round 5 evicted operands it had just checked).  The values may be shared secrets: wiped on every way out.
  struct Vals { int32_t v[2][40]; ~Vals() { explicit_bzero(v, sizeof(v)); } } vals;
  int32_t (*val)[40] = vals.v;
  bool readmit[2] = {false, false};
  for (int i = 0; i < nop; ++i) {
    if (hs[i] == 0) return fail(KYB_E_BAD_ARG, "deferred point: null handle");
    if (arena_id_of(hs[i]) == A.id) { opnd[i] = seq_of(hs[i]); continue; }
    int rc = dvalue(g, hs[i], val[i], nullptr);             // (locks the OTHER arena)
    if (rc) return rc;
    readmit[i] = true;
  }
  std::lock_guard<std::mutex> lk(A.mu);
  if (A.next_id >> H_SHIFT) return fail(KYB_E_BAD_ARG, "deferred point: this arena has handed out 2^40 handles");
  for (int i = 0; i < nop; ++i) {
    if (readmit[i]) continue;
    if (opnd[i] == 0) return fail(KYB_E_BAD_ARG, "deferred point: null handle");
    if (opnd[i] >= A.next_id) return fail(KYB_E_BAD_ARG, "deferred point: unknown handle");
    if (opnd[i] < A.first_id) {
      DeferArena::Kept* kp = A.kept_find(opnd[i]);
      if (!kp) return dcheck(A, opnd[i]);
      memcpy(val[i], kp->val, 160);
      readmit[i] = true;
    }
  }
  const uint64_t bound = evict_bound(g, A, 3);            // (3: this node and at most two operands taken in as leaves)
  for (int i = 0; i < nop; ++i) {
    if (readmit[i] || opnd[i] >= bound) continue;
    if (!(A.node(opnd[i])->flags & F_VAL)) { int rc = dflush(g, A, &opnd[i], 1, false); if (rc) return rc; }
    DHdr* n = A.node(opnd[i]);
    if (!n || !(n->flags & F_VAL)) return fail(KYB_E_BAD_ARG, "deferred point: the evaluation finished without a value for this handle (an engine defect, never a result)");
    memcpy(val[i], A.pay(*n)->val, 160);
    readmit[i] = true;
  }
  { int rc = make_room(g, A, 3); if (rc) return rc; }
  for (int i = 0; i < nop; ++i)
    if (readmit[i]) { int rc = dinput(g, A, val[i], &opnd[i]); if (rc) return rc; ++A.st_readmitted; }
  uint64_t id = 0;
  dnew(A, op, opnd[0], opnd[1], sc, &id);
  A.pending.push_back(id);
  *out = handle_of(A, id);
  return KYB_OK;
}
}  // namespace

extern "C" {
int kyb_defer_input_enc(const int32_t* ext, const uint8_t* enc, uint64_t* out) {
  ENTER_HOST();
  if (!ext || !out) return fail(KYB_E_BAD_ARG, "null argument");
  DeferArena& A = arena_of(g);
  std::lock_guard<std::mutex> lk(A.mu);
  uint64_t seq = 0;
  int rc = dinput(g, A, ext, &seq, enc);
  if (rc) return rc;
  *out = handle_of(A, seq);
  return KYB_OK;
}
int kyb_defer_input(const int32_t* ext, uint64_t* out) { return kyb_defer_input_enc(ext, nullptr, out); }
int kyb_defer_null(uint64_t* out) { return drecord(D_NULL, 0, 0, nullptr, out); }
int kyb_defer_base(uint64_t* out) { return drecord(D_BASE, 0, 0, nullptr, out); }
int kyb_defer_mul_base(const uint8_t* scalar, uint64_t* out) { if (!scalar) return fail(KYB_E_BAD_ARG, "null scalar"); return drecord(D_MULBASE, 0, 0, scalar, out); }
int kyb_defer_mul(const uint8_t* scalar, uint64_t p, uint64_t* out) { if (!scalar) return fail(KYB_E_BAD_ARG, "null scalar"); return drecord(D_MUL, p, 0, scalar, out); }
int kyb_defer_add(uint64_t a, uint64_t b, int subtract, uint64_t* out) { return drecord(subtract ? D_SUB : D_ADD, a, b, nullptr, out); }
int kyb_defer_neg(uint64_t a, uint64_t* out) { return drecord(D_NEG, a, 0, nullptr, out); }

int kyb_defer_flush(void) {
  ENTER_HOST();
  DeferArena& A = arena_of(g);
  std::lock_guard<std::mutex> lk(A.mu);
  return dflush(g, A, nullptr, 0, false);
}
int kyb_defer_get(uint64_t p, int32_t* out_ext, uint8_t* out_enc) {
  ENTER_HOST();
  return dvalue(g, p, out_ext, out_enc);
}
int kyb_defer_equal(uint64_t ha, uint64_t hb, uint8_t* eq) {
  ENTER_HOST();
  if (!eq) return fail(KYB_E_BAD_ARG, "null argument");
  if (ha == 0 || hb == 0) return fail(KYB_E_BAD_ARG, "deferred point: null handle");
  // the stack copies below may be Diffie-Hellman shared secrets: cleared on every return path, as drecord's Vals
  struct Copies { int32_t xa[40], xb[40]; uint8_t ea[32], eb[32]; ~Copies() { explicit_bzero(this, sizeof(*this)); } };
  if (arena_id_of(ha) != arena_id_of(hb)) {                 // points of two arenas: their limbs, then the ordinary comparison
    Copies cp;
    int32_t *xa = cp.xa, *xb = cp.xb;
    int rc = dvalue(g, ha, xa, nullptr); if (rc) return rc;
    rc = dvalue(g, hb, xb, nullptr); if (rc) return rc;
    return kyb_equal_batch(xa, xb, 1, eq);
  }
  std::shared_ptr<DeferArena> keep;
  DeferArena* own = g.defer.load(std::memory_order_acquire);
  if (own == nullptr || own->id != arena_id_of(ha)) {
    keep = arena_by_handle(ha);
    if (!keep) return fail(KYB_E_BAD_ARG, "deferred point: the arena that held this point is gone (its context was released long ago)");
    own = keep.get();
  }
  DeferArena& A = *own;
  std::lock_guard<std::mutex> lk(A.mu);
  const uint64_t a = seq_of(ha), b = seq_of(hb);
  if ((a != 0 && a < A.first_id) || (b != 0 && b < A.first_id)) {      // one of them lives in the table of kept values: limbs (evaluating the other if need be), then the ordinary comparison
    Copies cp;
    int32_t *xa = cp.xa, *xb = cp.xb;
    uint8_t *ea = cp.ea, *eb = cp.eb;
    auto fetch = [&](uint64_t q, int32_t* x, uint8_t* e, bool* has_enc) -> int {
      if (q < A.first_id) {
        DeferArena::Kept* k = A.kept_find(q);
        if (!k) return dcheck(A, q);
        memcpy(x, k->val, 160); *has_enc = k->has_enc != 0; if (*has_enc) memcpy(e, k->enc, 32);
        return KYB_OK;
      }
      int rc = dcheck(A, q); if (rc) return rc;
      if (!(A.node(q)->flags & F_VAL)) { rc = dflush(g, A, &q, 1, true); if (rc) return rc; }
      DHdr* n = A.node(q);
      if (!n || !(n->flags & F_VAL)) return fail(KYB_E_BAD_ARG, "deferred point: the evaluation finished without a value for this handle (an engine defect, never a result)");
      memcpy(x, A.pay(*n)->val, 160); *has_enc = (n->flags & F_ENC) != 0; if (*has_enc) memcpy(e, A.pay(*n)->enc, 32);
      return KYB_OK;
    };
    bool enc_a = false, enc_b = false;
    int rc = fetch(a, xa, ea, &enc_a); if (rc) return rc;
    rc = fetch(b, xb, eb, &enc_b); if (rc) return rc;
    if (enc_a && enc_b) { *eq = memcmp(ea, eb, 32) == 0; return KYB_OK; }
    ++A.st_calls;
    return kyb_equal_batch(xa, xb, 1, eq);
  }
  int rc = dcheck(A, a); if (rc) return rc;
  rc = dcheck(A, b); if (rc) return rc;
  // (the flush is asked for the encodings too: Point::eq compares encodings (point.rs:227-241), the kernels that evaluate the operands marshal them on the way
  //  with their shared inversion, and the marshal_binary that usually follows — verify_deal's caller hashes the share it has just checked — is a cache hit)
  if (!(A.node(a)->flags & F_VAL) || !(A.node(b)->flags & F_VAL)) { const uint64_t ts[2] = {a, b}; rc = dflush(g, A, ts, 2, true, true); if (rc) return rc; }
  DHdr *na = A.node(a), *nb = A.node(b);
  if (!na || !nb) return fail(KYB_E_BAD_ARG, "deferred point: left the arena while it was evaluated (an engine defect, never a result)");
  if (!(na->flags & F_VAL) || !(nb->flags & F_VAL)) return fail(KYB_E_BAD_ARG, "deferred point: the evaluation finished without a value for this handle (an engine defect, never a result)");
  if ((na->flags & F_ENC) && (nb->flags & F_ENC)) { *eq = memcmp(A.pay(*na)->enc, A.pay(*nb)->enc, 32) == 0; return KYB_OK; }
  ++A.st_calls;
  return kyb_equal_batch(A.pay(*na)->val, A.pay(*nb)->val, 1, eq);
}
uint64_t kyb_defer_mark(void) {
  Ctx* c = cur();
  if (c == nullptr || !c->ready) return 0;
  DeferArena& A = arena_of(*c);
  std::lock_guard<std::mutex> lk(A.mu);
  return handle_of(A, A.next_id);
}
int kyb_defer_floor(uint64_t mark) {
  ENTER_HOST();
  if (mark == 0) return KYB_OK;          // the mark of a thread that had recorded nothing (kyb_defer_mark without a context): nothing to drop
  std::shared_ptr<DeferArena> B = arena_by_handle(mark);
  if (!B) return fail(KYB_E_BAD_ARG, "kyb_defer_floor: not a mark of a living arena");
  DeferArena& A = *B;
  std::lock_guard<std::mutex> lk(A.mu);
  const uint64_t m = seq_of(mark) < A.next_id ? seq_of(mark) : A.next_id;
  while (A.first_id < m) A.drop_front();          // the host says it: values and all
  A.kept_drop_below(m);
  return KYB_OK;
}
int kyb_defer_stats(uint64_t* out, int cap) {
  ENTER_HOST();
  if (!out || cap < 1) return fail(KYB_E_BAD_ARG, "null argument");
  DeferArena& A = arena_of(g);
  std::lock_guard<std::mutex> lk(A.mu);
  const uint64_t v[12] = {A.st_nodes, A.st_flushes, A.st_calls, A.st_horner, A.st_sums, A.st_enc_hits, (uint64_t)A.size(), A.st_evicted,
                          (uint64_t)A.kept_at.size(), A.st_kept_dropped, A.st_kept_hits, A.st_readmitted};
  for (int i = 0; i < cap && i < 12; ++i) out[i] = v[i];
  return KYB_OK;
}
}  // extern "C"
