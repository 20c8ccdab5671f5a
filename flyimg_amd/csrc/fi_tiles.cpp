// fi_tiles.cpp -- the workgroup tiles of the streaming resample kernels
// (fi_runtime.h): k_rs_vr (persistent, block-major), k_rs_vm and k_rs_hv, with
// the band split and the XCD-aware order they share.
#include "fi_runtime.h"

using namespace fi;

static bool vr_debug() {
  static const bool on = getenv("FI_VR_DEBUG") != nullptr;
  return on;
}

// Bands of blocks: an image's nblk blocks are cut into bands only when the
// launch's nst strips alone would not reach `target` workgroups (at most
// `most` bands); band bnd of `bands` is blocks [band_start(bnd), band_start(bnd + 1)).
static int band_count(int64_t target, int64_t nst, int most) {
  const int bands = nst > 0 ? (int)((target + nst - 1) / nst) : 1;
  return std::max(1, std::min(bands, most));
}
static int band_start(int nblk, int bnd, int bands) { return (int)((int64_t)nblk * bnd / bands); }

// XCD-aware tile order of k_rs_vm and k_rs_hv: the tiles of one image go to
// one XCD queue (blockIdx % 8 under round-robin dispatch) back to back, so the
// halo columns its strips share hit that L2; the queues are then interleaved.
// With `lpt` (mixed batches: cfg4) the images go to the queues by LPT on their
// cost and each queue runs its costliest tiles first, so the launch does not
// end on one 24 MP image's strips; otherwise the images go round robin.
template <class Tile, class Cost>
static void xcd_order(const std::vector<std::vector<Tile>> &img_tiles, const std::vector<int64_t> &img_cost, bool lpt,
                      Cost cost, std::vector<Tile> *out) {
  const size_t n = img_tiles.size();
  // (cost, tile): each tile is costed once, and the sort moves these keys, not tiles
  std::vector<std::pair<int64_t, const Tile *>> q8[8];
  if (lpt && n > 1) {
    std::vector<int> order(n);
    for (size_t k = 0; k < n; k++) order[k] = (int)k;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return img_cost[x] > img_cost[y]; });
    int64_t load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int k : order) {
      const int x = (int)(std::min_element(load, load + 8) - load);
      load[x] += img_cost[k];
      for (const Tile &t : img_tiles[k]) q8[x].push_back({cost(t), &t});
    }
    for (auto &q : q8)
      std::stable_sort(q.begin(), q.end(), [](const auto &a, const auto &b) { return a.first > b.first; });
  } else {
    for (size_t k = 0; k < n; k++)
      for (const Tile &t : img_tiles[k]) q8[k % 8].push_back({0, &t});
  }
  size_t mx = 0, total = 0;
  for (auto &q : q8) {
    mx = std::max(mx, q.size());
    total += q.size();
  }
  out->reserve(out->size() + total);
  for (size_t i = 0; i < mx; i++)
    for (int x = 0; x < 8; x++)
      if (i < q8[x].size()) out->push_back(*q8[x][i].second);
}

// A vertical-first image of the batch: its VDesc, strips and tables.
struct VmWork {
  int32_t img, first_strip, nstrips;
  const VmV *V;
  const AxisTable *vt;
  int32_t hwsum2, hsh;
};
// k_rs_vr: images (their k_rs_vm VDesc, strips) with block-major tables.
struct VrWork {
  int32_t img, first_strip, nstrips;
  const VrV *V;
  int32_t hwsum2, hsh;  // the horizontal two-limb tables (fi_plan.h MfmaH::wsum2 / shift2)
};
// What one k_rs_vr launch over `work` depends on: the widest strip's LDS
// pitch, whether any image needs the Q16 output tile, the strips, and the most
// 16-px output blocks in a strip.
struct VrFacts {
  int vpitch = 0, max_nocb = 0;
  bool q16 = false;
  int64_t nstrips = 0;
};
static VrFacts vr_facts(const BatchPlan &Bp, const std::vector<VrWork> &work) {
  VrFacts F;
  for (const VrWork &w : work) {
    for (int st = 0; st < w.nstrips; st++) {
      F.vpitch = std::max(F.vpitch, Bp.vstrips[w.first_strip + st].vpitch);
      F.max_nocb = std::max(F.max_nocb, Bp.vstrips[w.first_strip + st].nocb);
    }
    const VDesc &d = Bp.vdescs[w.img];
    F.q16 = F.q16 || d.gray || d.rot != 0;
    F.nstrips += w.nstrips;
  }
  return F;
}
// k_rs_vr workgroups: tiles (image, strip, band of blocks) in the XCD-aware
// order of k_rs_vm, dealt round-robin to one persistent workgroup per CU; the
// tiles of a workgroup form its row stream.  False (nothing launched) when the
// ring does not fit LDS or a stream needs more rows resident than the ring has.
static bool build_vr_tiles(fi_ctx *c, Exec &E, BatchPlan &Bp, const std::vector<VrWork> &work, const VrFacts &F) {
  const int vpitch = F.vpitch;
  const bool q16 = F.q16;
  const int64_t nst = F.nstrips;
  VrLayout L = vr_lds_layout(vpitch, q16, 1);
  if (L.R <= 0) return false;
  // loader waves: 4 when every strip has one 16-px output block (3 items: one
  // per H wave).  Measured (round 5): cfg5 resize 8.45 -> 7.83 ms; cfg2 (two
  // blocks a strip, two items per H wave) neutral, cfg3 1 % slower, so they
  // keep 2.  FI_VR_NL=2 / 4 forces (4 only where it is valid: <= 2 blocks a
  // strip)
  {
    const int want = c->vr_nl ? c->vr_nl : (F.max_nocb <= 1 ? 4 : 2);
    L.nl = (want == 4 && F.max_nocb <= 2) ? 4 : 2;
  }
  // per image: a VDesc with the block-major tables
  std::vector<int32_t> desc_of(work.size());
  for (size_t k = 0; k < work.size(); k++) {
    const VrV &V = *work[k].V;
    auto vp = c->vr_at.find(&V);
    if (vp == c->vr_at.end()) {
      std::array<int32_t, 4> o;
      o[0] = E.put(V.rows);
      E.ai.insert(E.ai.end(), 32, 0);
      if (V.rstep == 0 && !V.rows.empty()) {
        // the uneven list again, as each k_rs_vr loader wave walks it (for 2
        // and for 4 loader waves): class rho = k mod C, entry j = the pair
        // (rows[C j + rho], rows[C j + rho + 1]), so a wave's own pairs (C = 2 NL
        // apart) are consecutive ints
        const int n = (int)V.rows.size(), J4 = vr_pair_cls_len(n, 4), J8 = vr_pair_cls_len(n, 8);
        std::vector<int32_t> pc(8 * (size_t)J4 + 16 * (size_t)J8);
        for (int C : {4, 8}) {
          const int J = C == 4 ? J4 : J8;
          for (int k = 0; k < C * J; k++) {  // the pair starting at list row k (fi_internal.h vr_pair_off)
            const size_t o = (size_t)(vr_pair_off(n, k, C) - (n + 32));
            pc[o] = V.rows[std::min(k, n - 1)];
            pc[o + 1] = V.rows[std::min(k + 1, n - 1)];
          }
        }
        E.put(pc);
      }
      E.align4();
      o[1] = E.put(V.bmeta);
      o[2] = E.put(V.w128);
      E.align4();
      o[3] = E.put(V.frag);
      vp = c->vr_at.emplace(&V, o).first;
    }
    VDesc m = Bp.vdescs[work[k].img];
    m.rows = vp->second[0];
    m.nrows = (int32_t)V.rows.size();
    m.row0 = V.row0;
    m.rstep = V.rstep;
    m.pmeta = vp->second[1];
    m.w128 = vp->second[2];
    m.frag = vp->second[3];
    m.nblk = V.nblk;
    m.vsh = V.shift;
    m.hsh = work[k].hsh;
    m.hwsum = work[k].hwsum2;
    desc_of[k] = (int32_t)Bp.vdescs.size();
    Bp.vdescs.push_back(m);
  }
  // per (tables, band): glen, the rows the band needs resident at once inside
  // it, Rend(b0) - kbase and K0(b1 - 1) - kbase (the seams between tiles)
  struct Span {
    int32_t glen, inner, head, tail;
  };
  HashMap<std::tuple<const VrV *, int, int>, Span> spans;
  std::tuple<const VrV *, int, int> last_key{nullptr, -1, -1};
  const Span *last_sp = nullptr;
  auto span_of = [&](const VrV &V, int b0, int b1) -> const Span & {
    const auto key = std::make_tuple(&V, b0, b1);
    if (last_sp && key == last_key) return *last_sp;  // consecutive images mostly share tables
    last_key = key;
    auto it = spans.find(key);
    if (it != spans.end()) return *(last_sp = &it->second);
    const int32_t *bm = V.bmeta.data();
    const int kbase = bm[4 * b0];
    Span sp{};
    sp.glen = (bm[4 * (b1 - 1) + 2] - kbase + 15) / 16 * 16;
    sp.head = bm[4 * b0 + 2] - kbase;
    sp.tail = bm[4 * (b1 - 1)] - kbase;
    sp.inner = sp.head;
    for (int b = b0; b + 1 < b1; b++) sp.inner = std::max(sp.inner, bm[4 * (b + 1) + 2] - bm[4 * b]);
    last_sp = &spans.emplace(key, sp).first->second;
    return *last_sp;
  };
  // tiles (image, strip, band of blocks), costed as the rows they stream plus
  // a per-phase overhead of 16 rows
  struct TC {
    VrTile t;
    int64_t cost;
    const Span *sp;
  };
  std::vector<TC> all;
  all.reserve((size_t)nst);
  // tiles of one (image, band) share a cost: groups [first, first + n) of `all`
  struct Grp {
    int64_t cost;
    int32_t first, n;
  };
  std::vector<Grp> grps;
  grps.reserve(work.size());
  std::vector<int64_t> img_cost(work.size(), 0);
  for (size_t k = 0; k < work.size(); k++) {
    const VrWork &w = work[k];
    const int nblk = w.V->nblk;
    const int bands = band_count(2048, nst, nblk);
    for (int bnd = 0; bnd < bands; bnd++) {
      const int b0 = band_start(nblk, bnd, bands), b1 = band_start(nblk, bnd + 1, bands);
      if (b1 <= b0) continue;
      const Span &sp = span_of(*w.V, b0, b1);
      if (sp.inner > L.R) {
        if (vr_debug()) fprintf(stderr, "vr reject: inner %d > R %d\n", sp.inner, L.R);
        return false;
      }
      const int64_t cost = sp.glen + 16 * (b1 - b0);
      grps.push_back(Grp{cost, (int32_t)all.size(), w.nstrips});
      for (int st = 0; st < w.nstrips; st++)
        all.push_back(TC{VrTile{desc_of[k], w.first_strip + st, b0, b1, 0, 0, 0, (int32_t)k}, cost, &sp});
      img_cost[k] += cost * w.nstrips;
    }
  }
  const int ntiles = (int)all.size();
  if (ntiles == 0) return false;
  VrLayout L1{};
  {
    // two Q16 plane buffers (by block parity: the V waves never wait for the H
    // waves' reads) cost the ring 32 rows; taken when the smaller ring still
    // holds every block's and its successor's rows with max(32, half a block
    // step) to spare.  Measured (round 5): cfg2 (33 spare) 1.99 -> 1.93 ms;
    // cfg3 (19) and cfg5 (3) slower.  FI_VR_PBUF=1 / 2 forces (2 where it fits)
    int inner = 0, step = 0;
    for (const auto &kv : spans) inner = std::max(inner, kv.second.inner);
    for (const VrWork &w : work) {
      const int32_t *bm = w.V->bmeta.data();
      for (int b = 0; b + 1 < w.V->nblk; b++) step = std::max(step, bm[4 * (b + 1)] - bm[4 * b]);
    }
    const VrLayout L2 = vr_lds_layout(vpitch, q16, 2);
    const int want = c->vr_pbuf ? c->vr_pbuf : (L2.R - inner >= std::max(32, step / 2) ? 2 : 1);
    L1 = L;
    if (want == 2 && L2.R >= inner) {
      L = L2;
      L.nl = L1.nl;
    }
  }
  int G = std::min(ntiles, c->n_cu);
  if (G > 8) G -= G % 8;
  // workgroup g runs on XCD g % 8; with fewer than 4 images per XCD (small
  // batches, the serving shape) the tiles spread over every workgroup instead
  const int nx = G >= 8 && work.size() >= 32 ? 8 : 1;
  // images -> XCDs by LPT on their cost (an image's strips share halo columns
  // in that XCD's L2), then each XCD's tiles -> its workgroups by LPT
  std::vector<int> order(work.size());
  for (size_t k = 0; k < work.size(); k++) order[k] = (int)k;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return img_cost[x] > img_cost[y]; });
  std::vector<int> xcd_of(work.size(), 0);
  {
    std::vector<int64_t> load(nx, 0);
    for (int k : order) {
      const int x = (int)(std::min_element(load.begin(), load.end()) - load.begin());
      xcd_of[k] = x;
      load[x] += img_cost[k];
    }
  }
  // equal costs (a uniform batch) keep the list order: no sort needed; else
  // LPT over the tiles longest first, sorting the (image, band) groups (the
  // tiles of a group cost the same) rather than the tiles
  bool uniform = true;
  for (const Grp &gp : grps) uniform = uniform && gp.cost == grps[0].cost;
  std::vector<const TC *> order_t;
  order_t.reserve(all.size());
  if (uniform) {
    for (const TC &tc : all) order_t.push_back(&tc);
  } else {
    std::stable_sort(grps.begin(), grps.end(), [](const Grp &x, const Grp &y) { return x.cost > y.cost; });
    for (const Grp &gp : grps)
      for (int i = 0; i < gp.n; i++) order_t.push_back(&all[gp.first + i]);
  }
  std::vector<std::vector<const TC *>> per(G);
  for (auto &v : per) v.reserve(ntiles / G + 8);
  if (uniform) {
    // equal costs: LPT is a round robin over each XCD's workgroups
    std::vector<int> next(nx, 0);
    const int per_x = G / nx;
    for (const TC *tc : order_t) {
      const int x = xcd_of[tc->t.pad];
      per[x + nx * (next[x]++ % per_x)].push_back(tc);
    }
  } else {
    // longest first, dealt boustrophedon over each XCD's workgroups (0 .. n-1,
    // n-1 .. 0, ...): O(1) per tile and, over ~80 sorted tiles per
    // workgroup, within a tile of LPT's balance (an LPT heap per tile cost
    // ~1 ms of host planning per cfg4 batch)
    std::vector<int> next(nx, 0);
    const int per_x = G / nx;
    for (const TC *tc : order_t) {
      const int x = xcd_of[tc->t.pad];
      const int i = next[x]++, r = i % per_x;
      per[x + nx * (((i / per_x) & 1) ? per_x - 1 - r : r)].push_back(tc);
    }
  }
  // the streams: workgroup g walks tiles [t0(g), t1(g)); every phase's rows
  // [K0, Rend) and the next phase's must be resident together
  std::vector<VrTile> tiles;
  std::vector<int32_t> info;
  auto streams = [&](int R) -> bool {
    tiles.clear();
    tiles.reserve(ntiles);
    info.assign(4 * (size_t)G, 0);
    for (int g = 0; g < G; g++) {
      int64_t gpos = 0, prev_tail = -1;
      info[4 * g + 2] = (int32_t)tiles.size();
      for (const TC *tc : per[g]) {
        VrTile T = tc->t;
        const VrV &V = *work[T.pad].V;
        const Span &sp = *tc->sp;
        T.kbase = V.bmeta[4 * T.b0];
        T.glen = sp.glen;
        T.g0 = (int32_t)gpos;
        // the seam: this tile's first block's rows and the previous tile's last
        // block's window resident together
        if (prev_tail >= 0 && T.g0 + sp.head - prev_tail > R) return false;
        prev_tail = T.g0 + sp.tail;
        info[4 * g] += T.b1 - T.b0;
        gpos += T.glen;
        if (gpos >= ((int64_t)1 << 30)) return false;
        T.pad = 0;
        tiles.push_back(T);
      }
      info[4 * g + 1] = (int32_t)gpos;
      info[4 * g + 3] = (int32_t)tiles.size();
    }
    return true;
  };
  if (!streams(L.R)) {
    if (L.pbuf != 2) {
      if (vr_debug()) fprintf(stderr, "vr reject: seam, R %d\n", L.R);
      return false;
    }
    L = L1;  // a seam needs the bigger ring
    if (!streams(L.R)) {
      if (vr_debug()) fprintf(stderr, "vr reject: seam, R %d (one plane buffer)\n", L.R);
      return false;
    }
  }
  if (vr_debug()) {
    int inner = 0, rpb = 0;
    const int nocb = F.max_nocb;
    for (const auto &kv : spans) inner = std::max(inner, kv.second.inner);
    for (const VrWork &w : work) {
      const int32_t *bm = w.V->bmeta.data();
      for (int b = 0; b + 1 < w.V->nblk; b++) rpb = std::max(rpb, bm[4 * (b + 1)] - bm[4 * b]);
    }
    int hist[4] = {0, 0, 0, 0};
    for (const VrTile &t : tiles) hist[std::min(3, Bp.vstrips[t.strip].nocb)]++;
    fprintf(stderr, "vr: R %d pbuf %d nl %d vpitch %d inner %d K0 step max %d nocb %d (tiles by nocb %d %d %d) tiles %d G %d\n",
            L.R, L.pbuf, L.nl, vpitch, inner, rpb, nocb, hist[1], hist[2], hist[3], ntiles, G);
  }
  Bp.vrl.push_back(BatchPlan::VrLaunch{(int32_t)Bp.vrtiles.size(), (int32_t)tiles.size(), (int32_t)Bp.vr_info.size(),
                                        G, (int32_t)work.size(), L});
  Bp.vrtiles.insert(Bp.vrtiles.end(), tiles.begin(), tiles.end());
  Bp.vr_info.insert(Bp.vr_info.end(), info.begin(), info.end());
  return true;
}

// per table: its first / last (+ pad) / widest block windows and its widest two
// consecutive blocks' rows (build_vr_tiles' `inner`)
using VrWindows = HashMap<const VrV *, std::array<int, 4>>;
// Consecutive tiles of a workgroup's stream hold the last block window of one
// and the first of the next in the ring together (the seam, build_vr_tiles),
// and one failing seam sends the whole launch to k_rs_vm.  Images leave `part`
// for `rest` (largest windows first) until the largest first window plus the
// largest last window fit the ring, so the rest chain in any order:
// whole-image tiles (>= 2048 strips: one band) by their edge blocks' windows,
// banded ones by their widest window.  True when any image left.
static bool drop_seam_misfits(const VrFacts &F, VrWindows &wmax_of, std::vector<VrWork> &part,
                              std::vector<VmWork> &part_w, std::vector<VmWork> &rest) {
  const int R = vr_lds_layout(F.vpitch, F.q16, 1).R;
  const bool whole = F.nstrips >= 2048;
  std::vector<std::array<int, 3>> hl(part.size());  // head, last window, index
  for (size_t k = 0; k < part.size(); k++) {
    const VrV &V = *part[k].V;
    auto wm = wmax_of.find(&V);
    if (wm == wmax_of.end()) {
      const int32_t *bm = V.bmeta.data();
      const int nb = V.nblk;
      int w = 0, inner = bm[2] - bm[0];
      for (int b = 0; b < nb; b++) w = std::max(w, bm[4 * b + 2] - bm[4 * b]);
      for (int b = 0; b + 1 < nb; b++) inner = std::max(inner, bm[4 * (b + 1) + 2] - bm[4 * b]);
      const int glen = (bm[4 * (nb - 1) + 2] - bm[0] + 15) / 16 * 16;
      wm = wmax_of.emplace(&V, std::array<int, 4>{bm[2] - bm[0], glen - (bm[4 * (nb - 1)] - bm[0]), w, inner}).first;
    }
    const auto &a = wm->second;
    // a tile's first window is its first block's, its last one (K0s are
    // multiples of 16) its last block's rounded up to 16 rows
    hl[k] = whole ? std::array<int, 3>{a[0], a[1], (int)k} : std::array<int, 3>{a[2], (a[2] + 15) / 16 * 16, (int)k};
    if (a[3] > R) hl[k] = {R + 1, R + 1, (int)k};  // a block pair alone exceeds the ring: always out
  }
  std::sort(hl.begin(), hl.end(), [](const std::array<int, 3> &x, const std::array<int, 3> &y) {
    return std::max(x[0], x[1]) > std::max(y[0], y[1]);
  });
  // the fewest leading (largest) images to drop: suffix maxima of both windows
  std::vector<int> sh(hl.size() + 1, 0), sl(hl.size() + 1, 0);
  for (size_t k = hl.size(); k-- > 0;) {
    sh[k] = std::max(sh[k + 1], hl[k][0]);
    sl[k] = std::max(sl[k + 1], hl[k][1]);
  }
  size_t drop = 0;
  while (drop < hl.size() && sh[drop] + sl[drop] > R) drop++;
  if (drop == 0) return false;
  std::vector<char> out(part.size(), 0);
  for (size_t k = 0; k < drop; k++) out[hl[k][2]] = 1;
  std::vector<VrWork> keep;
  std::vector<VmWork> keep_w;
  for (size_t k = 0; k < part.size(); k++) {
    if (out[k]) {
      rest.push_back(part_w[k]);
    } else {
      keep.push_back(part[k]);
      keep_w.push_back(part_w[k]);
    }
  }
  part.swap(keep);
  part_w.swap(keep_w);
  return true;
}

// k_rs_vm workgroups: (image, strip, band of blocks); the tables of a geometry
// are placed in the heap once.
void fi::build_vm_tiles(fi_ctx *c, Exec &E, BatchPlan &Bp) {
  HashMap<const MfmaH *, std::array<int32_t, 5>> hplaced;  // first strip, hwsum, hwsum2, LDS (8-bit / Q16 tile)
  std::vector<VmWork> work;
  const int nv = (int)Bp.vm_img.size();
  work.reserve(nv);
  Bp.vdescs.reserve(2 * (size_t)nv);  // + the k_rs_vr descriptors
  for (int q = 0; q < nv; q++) {
    const ResizeDesc &d = Bp.rd[Bp.vm_img[q]];
    const VmV &V = *Bp.vm_v[q];
    const MfmaH &H = *Bp.vm_h[q];
    auto vp = c->vv_at.find(&V);
    if (vp == c->vv_at.end()) {
      std::array<int32_t, 8> o;
      std::vector<int32_t> meta;
      for (size_t k = 0; k < V.plo.size(); k++) {
        meta.push_back(V.plo[k]);
        meta.push_back(V.pn[k]);
        meta.push_back(V.pblk[k]);
        meta.push_back(V.plast[k]);
      }
      E.align4();
      o[7] = E.put(meta);
      o[0] = E.put(V.rows);
      o[1] = E.put(V.plo);
      o[2] = E.put(V.pn);
      o[3] = E.put(V.pblk);
      o[4] = E.put(V.plast);
      E.align4();
      o[5] = E.put(V.w128);
      E.align4();
      o[6] = E.put(V.frag);
      vp = c->vv_at.emplace(&V, o).first;
    }
    auto hp = hplaced.find(&H);
    if (hp == hplaced.end()) {
      const int32_t first = (int32_t)Bp.vstrips.size();
      auto ht = c->mh_at.find(&H);
      if (ht == c->mh_at.end()) {
        fi_ctx::MhPlaced pl;
        pl.hwsum = E.put(H.wsum);
        E.align4();
        const int32_t frag = E.put(H.frag);
        const int32_t s0 = E.put(H.s0);
        E.align4();  // 16-byte aligned LUT rows (k_rs_vr's LDS-DMA)
        const int32_t lut = E.put(H.lut);
        E.align4();
        const int32_t frag2 = E.put(H.frag2);
        pl.hwsum2 = E.put(H.wsum2);
        pl.strips.reserve(H.strips.size());
        for (const MfmaStrip &st : H.strips) {
          MStrip m{};
          m.x0 = st.x0;
          m.x1 = st.x1;
          m.b0 = st.b0;
          m.nbytes = st.nbytes;
          m.c_lo = st.c_lo;
          m.ncols = st.ncols;
          m.pitch = st.pitch;
          m.nocb = st.nocb;
          m.ks = st.ks;
          m.lut_px0 = st.lut_px0;
          m.lut_n = st.lut_n;
          m.frag = frag + (int32_t)st.frag;
          m.s0 = s0 + (int32_t)st.s0;
          m.lut = lut + (int32_t)st.lut;
          m.vpitch = st.vpitch;
          m.frag2 = frag2 + (int32_t)st.frag2;
          pl.strips.push_back(m);
          // the workgroup's LDS layout follows its strip and tile kind
          pl.lds8 = std::max(pl.lds8, vm_lds_bytes(st.vpitch, st.nocb, st.ks, false));
          pl.lds16 = std::max(pl.lds16, vm_lds_bytes(st.vpitch, st.nocb, st.ks, true));
        }
        ht = c->mh_at.emplace(&H, std::move(pl)).first;
      }
      const fi_ctx::MhPlaced &pl = ht->second;
      Bp.vstrips.insert(Bp.vstrips.end(), pl.strips.begin(), pl.strips.end());
      hp = hplaced.emplace(&H, std::array<int32_t, 5>{first, pl.hwsum, pl.hwsum2, (int32_t)pl.lds8, (int32_t)pl.lds16})
               .first;
    }
    Bp.vm_lds = std::max(Bp.vm_lds, (size_t)hp->second[(d.gray || d.rot != 0) ? 4 : 3]);
    VDesc m{};
    m.src = d.src;
    m.src_stride = d.src_stride;
    m.dst = d.dst;
    m.dst_stride = d.dst_stride;
    m.ew = d.ew;
    m.eh = d.eh;
    m.rot = d.rot;
    m.gray = d.gray;
    m.rows = vp->second[0];
    m.nrows = (int32_t)V.rows.size();
    m.row0 = V.row0;
    m.rstep = V.rstep;
    m.plo = vp->second[1];
    m.pn = vp->second[2];
    m.pblk = vp->second[3];
    m.plast = vp->second[4];
    m.w128 = vp->second[5];
    m.frag = vp->second[6];
    m.pmeta = vp->second[7];
    m.hwsum = hp->second[1];
    m.nblk = V.nblk;
    work.push_back({(int32_t)Bp.vdescs.size(), hp->second[0], (int32_t)H.strips.size(), &V, Bp.vm_vt[q], hp->second[2],
                    H.shift2});
    Bp.vdescs.push_back(m);
  }
  // k_rs_vr (default; FI_VR_RS=0 turns it off): the images whose vertical axis has block-major
  // tables (fi_plan.h VrV) run on the persistent block-major kernel
  Bp.vrl.clear();
  Bp.vrtiles.clear();
  Bp.vr_info.clear();
  const double t_vr0 = now_ms();
  if (c->vr_rs) {
    std::vector<VmWork> rest;
    std::vector<VrWork> vr;
    std::vector<VmWork> vr_w;  // the VmWork of each vr entry (back to k_rs_vm if its launch cannot be built)
    for (const VmWork &w : work) {
      auto it = c->vrv_cache.find(w.vt);
      if (it == c->vrv_cache.end()) {
        VrV m;
        if (!build_vr_v(*w.vt, &m)) m = VrV();
        it = c->vrv_cache.emplace(w.vt, std::move(m)).first;
      }
      const VrV &V = it->second;
      const int64_t gap = V.maxgap;  // the DMA's per-lane row offset
      bool narrow = true;  // five H waves take two horizontal items each: <= 3 16-px blocks per strip
      for (int st = 0; st < w.nstrips; st++) narrow = narrow && Bp.vstrips[w.first_strip + st].nocb <= 3;
      if (V.nblk > 0 && w.hsh > 0 && narrow && gap * Bp.vdescs[w.img].src_stride < ((int64_t)1 << 31)) {
        vr.push_back({w.img, w.first_strip, w.nstrips, &V, w.hwsum2, w.hsh});
        vr_w.push_back(w);
      } else {
        rest.push_back(w);
      }
    }
    // mixed geometries (cfg4's 384 size classes x five ops) were slower on
    // k_rs_vr than on k_rs_vm in round 4 (432 vs 385 ms), hence a class cap
    // (FI_VR_MAX_CLASSES); since round 5 (4 loader waves for one-block strips,
    // their own launch) k_rs_vr takes them: cfg4 resize 363 -> 329 ms per step
    VrWindows wmax_of;
    std::vector<const VrV *> classes;
    classes.reserve(vr.size());
    for (const VrWork &w : vr) classes.push_back(w.V);
    std::sort(classes.begin(), classes.end());
    const int nclasses = (int)(std::unique(classes.begin(), classes.end()) - classes.begin());
    if (!vr.empty() && nclasses <= c->vr_max_classes) {
      // two launches when the batch mixes strips of one 16-px output block
      // (4 loader waves) with wider ones (2) and both halves fill the chip
      std::vector<int> grp(vr.size(), 0);
      int64_t nst[2] = {0, 0};
      for (size_t k = 0; k < vr.size(); k++) {
        int mx = 0;
        for (int st = 0; st < vr[k].nstrips; st++) mx = std::max(mx, Bp.vstrips[vr[k].first_strip + st].nocb);
        grp[k] = mx <= 1 ? 0 : 1;
        nst[grp[k]] += vr[k].nstrips;
      }
      const bool split = c->vr_split && nst[0] >= 2 * c->n_cu && nst[1] >= 2 * c->n_cu;
      for (int g = 0; g < (split ? 2 : 1); g++) {
        std::vector<VrWork> part;
        std::vector<VmWork> part_w;
        for (size_t k = 0; k < vr.size(); k++)
          if (!split || grp[k] == g) {
            part.push_back(vr[k]);
            part_w.push_back(vr_w[k]);
          }
        VrFacts F = vr_facts(Bp, part);
        if (drop_seam_misfits(F, wmax_of, part, part_w, rest)) F = vr_facts(Bp, part);
        if (!part.empty() && !build_vr_tiles(c, E, Bp, part, F)) rest.insert(rest.end(), part_w.begin(), part_w.end());
      }
      work.swap(rest);
    }
  }
  host_stat(c, "host_plan_vr", now_ms() - t_vr0);
  // bands of blocks only when the batch is too small to fill the chip
  int64_t nst = 0;
  for (const VmWork &w : work) nst += w.nstrips;
  // images cost their pieces (c->vm_lpt: xcd_order)
  std::vector<std::vector<VTile>> img_tiles(work.size());
  std::vector<int64_t> img_cost(work.size(), 0);
  for (size_t k = 0; k < work.size(); k++) {
    const VmWork &w = work[k];
    const VmV &V = *w.V;
    const int bands = band_count(2048, nst, V.nblk);
    std::vector<int> first_piece(V.nblk + 1, (int)V.plo.size());
    for (int p = (int)V.plo.size() - 1; p >= 0; p--) first_piece[V.pblk[p]] = p;
    for (int bnd = 0; bnd < bands; bnd++) {
      const int b0 = band_start(V.nblk, bnd, bands), b1 = band_start(V.nblk, bnd + 1, bands);
      if (b1 <= b0) continue;
      const int p0 = first_piece[b0 > 0 ? b0 - 1 : 0];
      const int p1 = first_piece[b1];
      for (int st = 0; st < w.nstrips; st++) {
        img_tiles[k].push_back(VTile{w.img, w.first_strip + st, p0, p1, b0, 0});
        img_cost[k] += p1 - p0 + 1;
      }
    }
  }
  xcd_order(img_tiles, img_cost, c->vm_lpt, [](const VTile &t) { return t.p1 - t.p0 + 1; }, &Bp.vtiles);
}

// k_rs_hv workgroups: (image, strip, band of output blocks); bands only when
// the horizontal-first images alone would not fill the chip (each band
// re-produces the intermediate rows of its first block's window).
void fi::build_hv_tiles(fi_ctx *c, Exec &E, BatchPlan &Bp) {
  HashMap<const HvH *, int32_t> splaced;  // first strip in Bp.hstrips
  struct Work1 {
    int32_t img, first_strip, nstrips, nblk, nrows;
  };
  std::vector<Work1> work;
  for (size_t q = 0; q < Bp.hv_img.size(); q++) {
    const ResizeDesc &d = Bp.rd[Bp.hv_img[q]];
    const HvV &V = *Bp.hv_v[q];
    const HvH &H = *Bp.hv_h[q];
    auto vp = c->hvv_at.find(&V);
    if (vp == c->hvv_at.end()) {
      std::array<int32_t, 3> o;
      o[0] = E.put(V.k0ks);
      E.align4();
      o[1] = E.put(V.frag);
      o[2] = E.put(V.wsum);
      vp = c->hvv_at.emplace(&V, o).first;
    }
    auto hp = c->hvh_at.find(&H);
    if (hp == c->hvh_at.end()) {
      std::array<int32_t, 3> o;
      o[0] = E.put(H.w128);
      E.align4();
      o[1] = E.put(H.frag);
      o[2] = E.put(H.s0);
      hp = c->hvh_at.emplace(&H, o).first;
    }
    auto sp = splaced.find(&H);
    if (sp == splaced.end()) {
      const int32_t first = (int32_t)Bp.hstrips.size();
      for (const HvStrip &st : H.strips) {
        HvStripD m{};
        m.x0 = st.x0;
        m.x1 = st.x1;
        m.px0 = st.px0;
        m.pp = st.pp;
        m.nocb = st.nocb;
        m.frag = hp->second[1] + (int32_t)st.frag;
        m.s0 = hp->second[2] + (int32_t)st.s0;
        Bp.hstrips.push_back(m);
        Bp.hv_lds = std::max(Bp.hv_lds, hv_lds_bytes(st.pp, st.nocb));
      }
      sp = splaced.emplace(&H, first).first;
    }
    HvDesc m{};
    m.src = d.src;
    m.src_stride = d.src_stride;
    m.dst = d.dst;
    m.dst_stride = d.dst_stride;
    m.ew = d.ew;
    m.eh = d.eh;
    m.rot = d.rot;
    m.gray = d.gray;
    m.row0 = V.row0;
    m.nrows = V.nrows;
    m.nblk = V.nblk;
    m.vk = vp->second[0];
    m.vfrag = vp->second[1];
    m.vws = vp->second[2];
    m.hw128 = hp->second[0];
    m.W = Bp.hv_W[q];
    work.push_back({(int32_t)Bp.hdescs.size(), sp->second, (int32_t)H.strips.size(), V.nblk, V.nrows});
    Bp.hdescs.push_back(m);
  }
  int64_t nst = 0;
  for (const Work1 &w : work) nst += w.nstrips;
  // tiles cost their share of the image's source rows (c->vm_lpt: xcd_order);
  // work[k] is the image of descriptor k: HvTile::img indexes both
  std::vector<std::vector<HvTile>> img_tiles(work.size());
  std::vector<int64_t> img_cost(work.size(), 0);
  auto tile_cost = [&](const HvTile &t) {
    const Work1 &w = work[t.img];
    return (int64_t)(t.b1 - t.b0) * w.nrows / std::max(w.nblk, 1) + 16;
  };
  for (size_t k = 0; k < work.size(); k++) {
    const Work1 &w = work[k];
    const int bands = band_count(8192, nst, w.nblk / 6);
    for (int bnd = 0; bnd < bands; bnd++) {
      const int b0 = band_start(w.nblk, bnd, bands), b1 = band_start(w.nblk, bnd + 1, bands);
      if (b1 <= b0) continue;
      for (int st = 0; st < w.nstrips; st++) {
        img_tiles[k].push_back(HvTile{w.img, w.first_strip + st, b0, b1});
        img_cost[k] += tile_cost(img_tiles[k].back());
      }
    }
  }
  xcd_order(img_tiles, img_cost, c->vm_lpt, tile_cost, &Bp.htiles);
}
