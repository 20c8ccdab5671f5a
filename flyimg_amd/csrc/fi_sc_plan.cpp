// fi_sc_plan.cpp -- the smartcrop stage of the runtime (fi_runtime.h): its
// planner (plans, crops, importance tables, k_sc_score3 groups), launch lists
// and enqueue, and the smartcrop-only entry points (fi_smartcrop / fi_smartcrop_ex).
#include "fi_runtime.h"

using namespace fi;

ScParamsDev fi::to_dev(const fi_smartcrop_params &p) {
  ScParamsDev d{};
  d.detail_weight = p.detail_weight;
  d.edge_radius = p.edge_radius;
  d.edge_weight = p.edge_weight;
  d.outside_importance = p.outside_importance;
  d.saturation_bias = p.saturation_bias;
  d.saturation_brightness_max = p.saturation_brightness_max;
  d.saturation_brightness_min = p.saturation_brightness_min;
  d.saturation_threshold = p.saturation_threshold;
  d.saturation_weight = p.saturation_weight;
  d.skin_bias = p.skin_bias;
  d.skin_brightness_max = p.skin_brightness_max;
  d.skin_brightness_min = p.skin_brightness_min;
  for (int i = 0; i < 3; i++) d.skin_color[i] = p.skin_color[i];
  d.skin_threshold = p.skin_threshold;
  d.skin_weight = p.skin_weight;
  d.rule_of_thirds = p.rule_of_thirds;
  return d;
}
static uint64_t params_hash(const fi_smartcrop_params &p) {
  const uint8_t *b = reinterpret_cast<const uint8_t *>(&p);
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < sizeof p; i++) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}

// k_sc_score3 groups of one plan's crops (fi_internal.h ScGroup): per
// importance table, the distinct x origins in chunks of 16 (M rows) times the
// y origins in chunks of kSgSlots (`step` apart: crops() walks a full grid per
// scale).  The plan keeps k_sc_score2 when any condition fails: more than
// kSgMax groups, x origins not 8-B aligned (two ds_read_b64 per fragment),
// windows wider than kSgMaxKs k-steps or of more than 2^17 pixels (int32
// sums of 2^14-bounded products), or planes beyond the LDS.
template <class ImpOf, class Placed>
static void plan_score_groups(fi_ctx *c, Exec &E, const ScPlan &P, int step, const ImpOf &imp_of, ScLaunchData *L,
                              Placed *q) {
  const size_t g0 = L->groups.size();
  std::vector<ScGroup> gs;
  std::vector<std::array<int, 3>> where(P.crops.size(), {-1, -1, -1});
  std::vector<std::pair<uint64_t, uint64_t>> order;
  for (const CropHost &ch : P.crops) {
    const auto k = std::make_pair(dbits(ch.fw), dbits(ch.fh));
    if (std::find(order.begin(), order.end(), k) == order.end()) order.push_back(k);
  }
  int tail = 0;
  for (const auto &k : order) {
    const auto &t = imp_of.at(k);
    const std::vector<double> *tab = std::get<0>(t);
    const int nx = std::get<1>(t), ny = std::get<2>(t);
    if ((int64_t)nx * ny >= (1 << 17)) return;
    std::vector<int> xs, ys;
    for (const CropHost &ch : P.crops)
      if (std::make_pair(dbits(ch.fw), dbits(ch.fh)) == k) {
        xs.push_back(ch.x0);
        ys.push_back(ch.y0);
      }
    std::sort(xs.begin(), xs.end());
    xs.erase(std::unique(xs.begin(), xs.end()), xs.end());
    std::sort(ys.begin(), ys.end());
    ys.erase(std::unique(ys.begin(), ys.end()), ys.end());
    for (size_t i = 1; i < ys.size(); i++)
      if (ys[i] - ys[i - 1] != step) return;
    for (int x : xs)
      if (x % 8) return;
    for (size_t xa = 0; xa < xs.size(); xa += 16)
      for (size_t ya = 0; ya < ys.size(); ya += kSgSlots) {
        const int nm = (int)std::min<size_t>(16, xs.size() - xa), nslot = (int)std::min<size_t>(kSgSlots, ys.size() - ya);
        const auto bk = std::make_tuple(tab, nx, nslot, step);
        auto bt = c->sgb_at.find(bk);
        if (bt == c->sgb_at.end()) {
          ScoreBTab b;
          sc_score_btab(*tab, nx, ny, E.params.outside_importance, nslot, step, &b);
          int32_t off = -1;
          if (b.ok) {
            while (E.ai.size() % 4) E.ai.push_back(0);  // 16-B aligned fragments
            off = E.oi();
            E.ai.insert(E.ai.end(), b.frag.begin(), b.frag.end());
          }
          b.frag.clear();
          bt = c->sgb_at.emplace(bk, std::make_pair(off, std::move(b))).first;
        }
        const ScoreBTab &b = bt->second.second;
        if (!b.ok) return;
        ScGroup g{};
        g.bfrag = bt->second.first;
        g.nrows = b.nrows;
        g.ks = b.ks;
        g.ybase = ys[ya];
        g.nm = nm;
        g.nslot = nslot;
        g.q = b.q;
        g.step = step;
        for (int m = 0; m < 16; m++) g.x0[m] = xs[xa + std::min(m, nm - 1)];
        for (int i = 0; i < kSgDigits; i++) g.S[i] = b.S[i];
        tail = std::max(tail, g.x0[nm - 1] + 64 * g.ks);
        for (size_t ci = 0; ci < P.crops.size(); ci++) {
          const CropHost &ch = P.crops[ci];
          if (std::make_pair(dbits(ch.fw), dbits(ch.fh)) != k) continue;
          const auto xi = std::find(xs.begin() + xa, xs.begin() + xa + nm, ch.x0);
          const int yi = (ch.y0 - ys[ya]) / step;
          if (xi == xs.begin() + xa + nm || ch.y0 < ys[ya] || yi >= nslot) continue;
          where[ci] = {(int)gs.size(), (int)(xi - (xs.begin() + xa)), yi};
        }
        gs.push_back(g);
      }
  }
  if (gs.empty() || (int)gs.size() > kSgMax) return;
  // LDS: the seven planes (rows of sg_pitch(aw) bytes) and what the last row's
  // widest fragment reads past them; the maps (exact re-score) and the
  // cross-wave sums reuse the same space
  const int pitch = sg_pitch(P.aw);
  const int64_t lds = std::max<int64_t>({(int64_t)kSgPlanes * P.ah * pitch + std::max(0, tail - pitch) + 16,
                                         (int64_t)P.aw * P.ah * 4, (int64_t)gs.size() * kSgPlanes * 1024});
  if (lds > kScore3Lds) return;
  for (size_t ci = 0; ci < P.crops.size(); ci++) {
    if (where[ci][0] < 0) return;
    DevCrop &dc = L->crops[q->crop0 + ci];
    dc.sg = where[ci][0];
    dc.sm = where[ci][1];
    dc.sj = where[ci][2];
  }
  q->sg0 = (int32_t)g0;
  q->nsg = (int32_t)gs.size();
  q->sg_lds = (int32_t)((lds + 15) & ~15);
  L->groups.insert(L->groups.end(), gs.begin(), gs.end());
}

// Plan the smartcrop stage of `items` into E (descriptors, crops, tables,
// workspace).  Per-item status in status[].  Images sharing a plan (same
// geometry) share its tables and crop list; `want_pre` keeps the prescaled
// image in the workspace (fi_smartcrop_ex).
void fi::plan_smartcrop(fi_ctx *c, Exec &E, const std::vector<ScItem> &items, ScLaunchData *L,
                           std::vector<int> *status, std::vector<std::string> *errs, bool want_pre) {
  const uint64_t ph = params_hash(E.params);
  // the fast pass's error bound assumes non-negative per-pixel terms
  const bool fast_ok = E.params.skin_bias >= 0 && E.params.saturation_bias >= 0;
  struct Placed {  // per batch: the plan's crop list in this batch's crop array
    int32_t crop0 = 0, ncrops = 0;
    int32_t sg0 = 0, nsg = 0, sg_lds = 0;  // k_sc_score3 groups (nsg = 0: k_sc_score2)
  };
  std::map<const ScPlan *, Placed> placed;
  for (size_t k = 0; k < items.size(); k++) {
    const ScItem &it = items[k];
    const fi_smartcrop_options &o = it.opt;
    uint64_t okey = dbits(o.max_scale) ^ (dbits(o.min_scale) * 3) ^ (dbits(o.scale_step) * 7) ^
                    ((uint64_t)o.step << 40) ^ ((uint64_t)o.prescale << 56);
    auto key = std::make_tuple(it.W, it.H, it.tw, it.th, okey);
    auto pit = c->sc_cache.find(key);
    if (pit == c->sc_cache.end()) {
      ScPlan p;
      plan_sc(it.W, it.H, it.tw, it.th, o, &p);
      pit = c->sc_cache.emplace(key, std::move(p)).first;
    }
    const ScPlan &P = pit->second;
    L->plans.push_back(&P);
    ScDesc d{};
    d.result = it.result;
    if (P.status != FI_OK) {
      (*status)[k] = P.status;
      (*errs)[k] = P.err;
      L->descs.push_back(d);
      continue;
    }
    auto pp = placed.find(&P);
    if (pp == placed.end()) {
      Placed q;
      auto tp = c->sc_at.find(&P);
      if (tp == c->sc_at.end()) {
        fi_ctx::ScTabs t;
        if (P.thumb) {
          t.hb = E.oi();
          E.ai.insert(E.ai.end(), P.hb.begin(), P.hb.end());
          t.hk = E.oi();
          E.ai.insert(E.ai.end(), P.hk.begin(), P.hk.end());
          t.hkT = E.oi();
          E.ai.insert(E.ai.end(), P.hkT.begin(), P.hkT.end());
          t.vb = E.oi();
          E.ai.insert(E.ai.end(), P.vb.begin(), P.vb.end());
          t.vk = E.oi();
          E.ai.insert(E.ai.end(), P.vk.begin(), P.vk.end());
          if (P.hm_ok) {
            while (E.ai.size() % 4) E.ai.push_back(0);  // 16-B aligned fragments
            t.hmB = E.oi();
            E.ai.insert(E.ai.end(), P.hmB.begin(), P.hmB.end());
            t.hmC = E.oi();
            E.ai.insert(E.ai.end(), P.hmC.begin(), P.hmC.end());
            t.hmS0 = E.oi();
            E.ai.insert(E.ai.end(), P.hmS0.begin(), P.hmS0.end());
          }
          if (P.vq_ok) {
            while (E.ai.size() % 4) E.ai.push_back(0);  // 16-B aligned fragments
            t.vqA = E.oi();
            E.ai.insert(E.ai.end(), P.vqA.begin(), P.vqA.end());
            t.vqK0 = E.oi();
            E.ai.insert(E.ai.end(), P.vqK0.begin(), P.vqK0.end());
          }
          if (P.vq_ok || P.cx_ok) {
            t.vqC = E.oi();
            E.ai.insert(E.ai.end(), P.vqC.begin(), P.vqC.end());
          }
          if (P.cx_ok) {
            while (E.ai.size() % 4) E.ai.push_back(0);  // 16-B aligned fragments
            t.cxA = E.oi();
            E.ai.insert(E.ai.end(), P.cxA.begin(), P.cxA.end());
            t.cxK0 = E.oi();
            E.ai.insert(E.ai.end(), P.cxK0.begin(), P.cxK0.end());
          }
        }
        tp = c->sc_at.emplace(&P, t).first;
      }
      // crops + importance tables (one table per distinct window size)
      std::map<std::pair<uint64_t, uint64_t>, std::pair<int, int>> sizes;
      for (const CropHost &ch : P.crops) {
        auto &e = sizes[{dbits(ch.fw), dbits(ch.fh)}];
        e.first = std::max(e.first, ch.nin_x);
        e.second = std::max(e.second, ch.nin_y);
      }
      std::map<std::pair<uint64_t, uint64_t>, std::tuple<int32_t, int32_t, double>> tab_of;
      std::map<std::pair<uint64_t, uint64_t>, std::pair<int32_t, double>> tab2_of;  // importance - oi
      std::map<std::pair<uint64_t, uint64_t>, std::tuple<const std::vector<double> *, int, int>> imp_of;
      for (auto &sz : sizes) {
        double fw, fh;
        memcpy(&fw, &sz.first.first, 8);
        memcpy(&fh, &sz.first.second, 8);
        const int nx = std::max(sz.second.first, 1), ny = std::max(sz.second.second, 1);
        auto ikey = std::make_tuple(sz.first.first, sz.first.second, nx, ny, ph);
        auto iit = c->imp_cache.find(ikey);
        if (iit == c->imp_cache.end()) {
          std::vector<double> t;
          sc_importance_table(E.params, fw, fh, nx, ny, &t);
          iit = c->imp_cache.emplace(ikey, std::move(t)).first;
        }
        auto pk = std::make_pair(&iit->second, nx);
        auto ip = c->imp_at.find(pk);
        if (ip == c->imp_at.end()) {
          double imax = 0;
          for (double v : iit->second) imax = std::max(imax, std::fabs(v));
          const int32_t off = E.od();
          E.ad.insert(E.ad.end(), iit->second.begin(), iit->second.end());
          ip = c->imp_at.emplace(pk, std::make_pair(off, imax)).first;
        }
        tab_of[sz.first] = std::make_tuple(ip->second.first, nx, ip->second.second);
        // the fast pass weighs inside pixels by fl(importance - oi): the outside
        // ones then need no pass (k_sc_score2)
        auto i2 = c->imp2_at.find(pk);
        if (i2 == c->imp2_at.end()) {
          double imax2 = 0;
          const int32_t off = E.od();
          const int nx2 = (nx + 63) / 64 * 64;  // rows padded with zeros: k_sc_score2's idle lanes weigh 0
          for (int y = 0; y < ny; y++) {
            for (int x = 0; x < nx; x++) {
              const double w = iit->second[(size_t)y * nx + x] - E.params.outside_importance;
              imax2 = std::max(imax2, std::fabs(w));
              E.ad.push_back(w);
            }
            E.ad.insert(E.ad.end(), (size_t)(nx2 - nx), 0.0);
          }
          i2 = c->imp2_at.emplace(pk, std::make_pair(off, imax2)).first;
        }
        tab2_of[sz.first] = i2->second;
        imp_of[sz.first] = std::make_tuple(&iit->second, nx, ny);
      }
      q.crop0 = (int32_t)L->crops.size();
      q.ncrops = (int32_t)P.crops.size();
      for (const CropHost &ch : P.crops) {
        DevCrop dc{};
        dc.fx = ch.fx;
        dc.fy = ch.fy;
        dc.fw = ch.fw;
        dc.fh = ch.fh;
        dc.x0 = ch.x0;
        dc.y0 = ch.y0;
        dc.nin_x = ch.nin_x;
        dc.nin_y = ch.nin_y;
        const auto &t = tab_of[{dbits(ch.fw), dbits(ch.fh)}];
        dc.table = std::get<0>(t);
        dc.table_w = std::get<1>(t);
        dc.imax = std::get<2>(t);
        dc.table2 = tab2_of[{dbits(ch.fw), dbits(ch.fh)}].first;
        dc.table2_w = (dc.table_w + 63) / 64 * 64;
        dc.imax2 = tab2_of[{dbits(ch.fw), dbits(ch.fh)}].second;
        dc.rx = ch.rx;
        dc.ry = ch.ry;
        dc.rw = ch.rw;
        dc.rh = ch.rh;
        dc.sg = dc.sm = dc.sj = -1;
        L->crops.push_back(dc);
      }
      if (fast_ok) plan_score_groups(c, E, P, o.step, imp_of, L, &q);
      pp = placed.emplace(&P, q).first;
    }
    const Placed &q = pp->second;
    const fi_ctx::ScTabs &T = c->sc_at.at(&P);
    // the per-image kernels (k_sc_fz; k_sc_hmfma + k_sc_vq, or k_sc_vmaps when the
    // vertical window exceeds one MFMA block), else the generic per-row kernels
    const bool prep = c->sc_prep && P.prep_ok && P.hm_ok;
    d.img = it.img;
    d.stride = it.stride;
    d.W = it.W;
    d.H = it.H;
    d.C = it.C;
    d.fx = P.fx;
    d.fy = P.fy;
    d.rw = P.rw;
    d.rh = P.rh;
    d.need_h = P.need_h;
    d.need_v = P.need_v;
    d.aw = P.aw;
    d.ah = P.ah;
    d.ybox_first = P.ybox_first;
    d.hrows = P.hrows;
    d.ksh = P.ksh;
    d.ksv = P.ksv;
    d.hb = T.hb;
    d.hk = T.hk;
    d.hkT = T.hkT;
    d.vb = T.vb;
    d.vk = T.vk;
    d.prep = prep ? 1 : 0;
    d.hm = prep ? 1 : 0;
    d.hm_rows = P.hm_rows;
    d.hm_ks = P.hm_ks;
    d.hm_pitch = P.hm_pitch;
    d.hm_nb = P.hm_nb;
    d.hmB = T.hmB;
    d.hmC = T.hmC;
    d.hmS0 = T.hmS0;
    d.vq = prep && P.vq_ok ? 1 : 0;
    d.fz = d.vq && P.fz_ok && c->sc_fz ? 1 : 0;
    d.fd = d.fz && c->sc_fd && it.C == 3 && it.stride % 16 == 0 && (it.padded || (it.W * 3) % 16 == 0) &&
                   P.hm_nb <= kFdCWaves &&
                   fd_lds(it.W, P.hm_pitch, P.aw, P.ah) <= kFdMaxLds
               ? 1
               : 0;
    d.vqA = T.vqA;
    d.vqC = T.vqC;
    d.vqK0 = T.vqK0;
    // k_sc_hx + k_sc_vx: their tables, the horizontal ones at <= 2 k-steps, rows
    // readable to the 16-B rounded row bytes (3 or 1 channels; the source's own
    // alignment is checked at launch)
    const int rowb = it.C == 3 ? fd_rp(it.W) : (it.W + 15) / 16 * 16;
    d.cx = prep && c->sc_cx > 0 && P.cx_ok && T.cxA >= 0 && P.fx == 1 && P.fy == 1 &&
                   (it.C == 3 || it.C == 1) && P.hm_ks <= 2 && it.stride % 16 == 0 &&
                   (it.padded || it.W * it.C == rowb)
               ? 1
               : 0;
    d.cx_kv = P.cx_kv;
    d.cx_tp = P.cx_tp;
    d.cxA = T.cxA;
    d.cxK0 = T.cxK0;
    d.prescale = P.prescale;
    d.exact_all = o.exact_all || !fast_ok;
    // workspace (offsets; converted to pointers after allocation)
    auto take = [&](size_t n) { return (uint8_t *)(uintptr_t)(E.work.take(n) + 1); };
    if (P.fx > 1 || P.fy > 1) d.red = take((size_t)P.rw * P.rh * 3);
    if (P.thumb && P.need_h && !d.fz)  // generic kernels: pitch aw*3; k_sc_hmfma: pitch apitch
      d.hbuf = take((size_t)(prep ? (P.aw * 3 + 15) / 16 * 16 : P.aw * 3) * std::max(P.hrows, 1));
    if (P.thumb && (!prep || want_pre)) d.pre = take((size_t)P.aw * P.ah * 3);
    if (d.cx) d.tbuf = take((size_t)P.hm_nb * it.C * 16 * P.cx_tp);
    d.maps = (uint32_t *)take((size_t)P.aw * P.ah * 4);
    d.crop0 = q.crop0;
    d.ncrops = q.ncrops;
    d.sg0 = q.sg0;
    d.ngrp = c->sc_mf ? q.nsg : 0;
    d.sg_lds = q.sg_lds;
    d.score0 = L->nscores;
    L->nscores += q.ncrops;
    L->descs.push_back(d);
  }
}
void fi::add_sc_launches(fi_ctx *c, Blob &B, const ScLaunchData &SL, const std::vector<int> &sstatus,
                            ScLaunches *X) {
  std::vector<int> sred, shp, svp, smaps;
  std::vector<ScDesc> hm, sl, sg, vq, vm, fz, fd, s3, cx;
  for (size_t k = 0; k < SL.descs.size(); k++) {
    if (sstatus[k] != FI_OK) continue;
    X->nok++;
    const ScDesc &d = SL.descs[k];
    const ScPlan &P = *SL.plans[k];
    if (d.red) sred.push_back((int)k);
    const bool aligned = ((uintptr_t)d.img & 15) == 0;
    const bool fd_ok = d.fz && d.fd && aligned;
    // k_sc_fd where it streams the image (cfg2: 0.353 vs k_sc_hx + k_sc_vx's
    // 0.44 ms per 1024 images), k_sc_fz where it does not, k_sc_hx +
    // k_sc_vx for gray sources in place of the k_sc_hmfma + k_sc_vq /
    // k_sc_vmaps pair (cfg5: 0.137 vs 0.586 ms per 1024 images); RGB keeps the
    // pair (cfg4 sc_prep 20.1 vs 22.6 ms per step with the RGB forms at 128
    // VGPRs and row-segmented tiles; 30.0 when they spilled at 64)
    // (FI_SC_CX=2, 3: first)
    if (d.cx && aligned && (c->sc_cx >= 2 || (d.C == 1 && !(fd_ok || d.fz)))) {
      cx.push_back(d);
    } else if (fd_ok) {
      fd.push_back(d);
      X->fd_lds = std::max(X->fd_lds, fd_lds(d.W, d.hm_pitch, d.aw, d.ah));
    } else if (d.fz) {
      fz.push_back(d);
      X->fz_lds = std::max(X->fz_lds, P.fz_lds);
    } else if (d.prep) {
      if (d.vq) {
        vq.push_back(d);
        X->vq_chunks = std::max(X->vq_chunks, P.vq_chunks);
        X->vq_lds = std::max(X->vq_lds, P.vq_lds);
      } else {
        vm.push_back(d);
        X->v_chunks = std::max(X->v_chunks, P.v_chunks);
        X->v_lds = std::max(X->v_lds, P.v_lds);
      }
      hm.push_back(d);
      X->hm_chunks = std::max(X->hm_chunks, P.hm_chunks);
      X->hm_lds = std::max(X->hm_lds, P.hm_lds);
    } else {
      if (d.hbuf) shp.push_back((int)k);
      if (d.pre) svp.push_back((int)k);
      smaps.push_back((int)k);
    }
    if (d.ngrp > 0) {
      s3.push_back(d);
      X->s3_lds = std::max(X->s3_lds, d.sg_lds);
    } else if ((int64_t)d.aw * d.ah * 4 <= kScoreLdsMaps) {
      sl.push_back(d);
      X->sl_px = std::max(X->sl_px, d.aw * d.ah);
    } else {
      sg.push_back(d);
    }
  }
  X->red = add_launch(B, SL.descs, sred, [](const ScDesc &d) { return d.rh; });
  X->hp = add_launch(B, SL.descs, shp, [](const ScDesc &d) { return d.hrows; });
  X->vp = add_launch(B, SL.descs, svp, [](const ScDesc &d) { return d.ah; });
  X->maps = add_launch(B, SL.descs, smaps, [](const ScDesc &d) { return d.ah; });
  X->hm_off = B.addv(hm);
  X->nhm = (int)hm.size();
  X->vq_off = B.addv(vq);
  X->vm_off = B.addv(vm);
  X->nvm = (int)vm.size();
  X->nvq = (int)vq.size();
  X->fz_off = B.addv(fz);
  X->nfz = (int)fz.size();
  X->fd_off = B.addv(fd);
  X->nfd = (int)fd.size();
  // k_sc_hx tiles (descriptor, first of 4 column blocks, first of kHxRb row blocks), k_sc_vx tiles
  // (descriptor, chunk) four to a workgroup, one list per variant
  X->cx_off = B.addv(cx);
  X->ncx = (int)cx.size();
  for (int v = 0; v < 4; v++) {
    const int ks = v / 2 + 1, nch = (v & 1) ? 3 : 1;
    std::vector<int32_t> ht, vt;
    for (size_t k = 0; k < cx.size(); k++) {
      const ScDesc &d = cx[k];
      if (d.C != nch) continue;
      if (d.hm_ks == ks)
        for (int r = 0; r < d.cx_tp / 16 - 1; r += kHxRb)
          for (int b = 0; b < d.hm_nb; b += 4) {
            ht.push_back((int32_t)k);
            ht.push_back(b);
            ht.push_back(r);
          }
      if (d.cx_kv == ks)
        for (int ch = 0; ch < (d.ah + kVqRows - 1) / kVqRows; ch++) {
          vt.push_back((int32_t)k);
          vt.push_back(ch);
        }
    }
    while (vt.size() % 8) {
      vt.push_back(-1);
      vt.push_back(0);
    }
    X->hxt_off[v] = B.addv(ht);
    X->hx_tiles[v] = (int)(ht.size() / 3);
    X->vxt_off[v] = B.addv(vt);
    X->vx_tiles[v] = (int)(vt.size() / 2);
  }
  c->stats["sc_path_cx"].launches += X->ncx;
  // images per smartcrop prescale kernel (fi_kernel_stats)
  c->stats["sc_path_fd"].launches += X->nfd;
  c->stats["sc_path_fz"].launches += X->nfz;
  X->sl_off = B.addv(sl);
  X->nsl = (int)sl.size();
  X->sg_off = B.addv(sg);
  X->nsg = (int)sg.size();
  X->s3_off = B.addv(s3);
  X->ns3 = (int)s3.size();
  c->stats["sc_score_mfma"].launches += X->ns3;  // images per score kernel (fi_kernel_stats)
  c->stats["sc_score_valu"].launches += X->nsl + X->nsg;
  X->groups_off = B.addv(SL.groups);
  X->crops_off = B.addv(SL.crops);
}
int fi::enqueue_sc(fi_ctx *c, hipStream_t st, uint8_t *ab, const ScLaunches &X, const int32_t *ai,
                      const double *ad, CropScore *scores, ScResult *results, const ScParamsDev &PD) {
  auto desc = [&](const Launch &L) { return (const ScDesc *)(ab + L.desc_off); };
  auto pre = [&](const Launch &L) { return (const int32_t *)(ab + L.prefix_off); };
  // the skin / saturation table of this parameter set (k_sc_fz), built
  // on the stream that reads it, so batches queued before a parameter change
  // have read the old table first
  const uint16_t *skinsat = nullptr;
  if (X.nfz > 0 || X.nfd > 0 || X.ncx > 0) {
    const std::string key(reinterpret_cast<const char *>(&PD), offsetof(ScParamsDev, pad));
    if (!c->skinsat.p || c->skinsat_key != key) {
      const int rc = ensure(c, &c->skinsat, (size_t)2 << 24);
      if (rc != FI_OK) return rc;
      // readers of the old table may still run on the other stream
      if (c->ap_pending && st == c->stream && order_after_apply(c) != FI_OK) return FI_EDEVICE;
      launch_sc_skinsat(st, (uint16_t *)c->skinsat.p, PD);
      c->skinsat_key = key;
    }
    skinsat = (const uint16_t *)c->skinsat.p;
  }
  {
    Timer t(c, "sc_prep", 0, st, st);
    if (X.red.tiles)
      hipLaunchKernelGGL(k_sc_reduce, dim3(X.red.tiles), dim3(256), 0, st, desc(X.red), pre(X.red), X.red.n);
    if (launch_sc_h(st, (const ScDesc *)(ab + X.hm_off), X.nhm, X.hm_chunks, X.hm_lds, ai) != 0 ||
        launch_sc_vq(st, (const ScDesc *)(ab + X.vq_off), X.nvq, X.vq_chunks, X.vq_lds, ai, PD) != 0 ||
        launch_sc_v(st, (const ScDesc *)(ab + X.vm_off), X.nvm, X.v_chunks, X.v_lds, ai, PD) != 0 ||
        launch_sc_fz(st, (const ScDesc *)(ab + X.fz_off), X.nfz, X.fz_lds, ai, PD, skinsat) != 0 ||
        launch_sc_fd(st, (const ScDesc *)(ab + X.fd_off), X.nfd, X.fd_lds, ai, PD, skinsat) != 0)
      return set_err(FI_EDEVICE, "smartcrop prescale launch rejected (LDS %d/%d/%d/%d)", X.hm_lds, X.vq_lds,
                     X.fz_lds, X.fd_lds);
    for (int v = 0; v < 4; v++) {
      const ScDesc *cd = (const ScDesc *)(ab + X.cx_off);
      if (launch_sc_hx(st, v / 2 + 1, (v & 1) ? 3 : 1, cd, (const int32_t *)(ab + X.hxt_off[v]), X.hx_tiles[v],
                       ai) != 0)
        return set_err(FI_EDEVICE, "k_sc_hx launch rejected");
    }
    for (int v = 0; v < 4; v++) {
      const ScDesc *cd = (const ScDesc *)(ab + X.cx_off);
      if (launch_sc_vx(st, v / 2 + 1, (v & 1) ? 3 : 1, cd, (const int32_t *)(ab + X.vxt_off[v]), X.vx_tiles[v],
                       ai, PD, skinsat) != 0)
        return set_err(FI_EDEVICE, "k_sc_vx launch rejected");
    }
    if (X.hp.tiles)
      hipLaunchKernelGGL(k_sc_hpass, dim3(X.hp.tiles), dim3(256), 0, st, desc(X.hp), pre(X.hp), X.hp.n, ai);
    if (X.vp.tiles)
      hipLaunchKernelGGL(k_sc_vpass, dim3(X.vp.tiles), dim3(256), 0, st, desc(X.vp), pre(X.vp), X.vp.n, ai);
    if (X.maps.tiles)
      hipLaunchKernelGGL(k_sc_maps, dim3(X.maps.tiles), dim3(256), 0, st, desc(X.maps), pre(X.maps),
                         X.maps.n, PD);
  }
  {
    Timer t(c, "sc_score", 0, st, st);
    const DevCrop *crops = (const DevCrop *)(ab + X.crops_off);
    if (launch_sc_score(st, 1, (const ScDesc *)(ab + X.sl_off), X.nsl, (size_t)X.sl_px * 4, crops, ad, scores,
                        results, PD, ai) != 0)
      return set_err(FI_EDEVICE, "k_sc_score2 launch rejected (%d px)", X.sl_px);
    (void)launch_sc_score(st, 0, (const ScDesc *)(ab + X.sg_off), X.nsg, 0, crops, ad, scores, results, PD, ai);
    if (launch_sc_score3(st, (const ScDesc *)(ab + X.s3_off), X.ns3, (size_t)X.s3_lds, crops,
                         (const ScGroup *)(ab + X.groups_off), ad, scores, results, PD, ai) != 0)
      return set_err(FI_EDEVICE, "k_sc_score3 launch rejected (%d B LDS)", X.s3_lds);
  }
  HIP_TRY(hipGetLastError());
  return FI_OK;
}

static int run_smartcrop(fi_ctx *c, const uint8_t *d_img, int W, int H, int64_t stride, int C, int tw, int th,
                         const fi_smartcrop_params &params, const fi_smartcrop_options &opt,
                         std::vector<CropScore> *scores, ScResult *result, ScPlan *plan_out,
                         std::vector<uint8_t> *prescaled, std::vector<uint8_t> *maps) {
  Exec E;
  E.c = c;
  E.params = params;
  {
    const int hrc = heap_prepare(c, E);
    if (hrc) return hrc;
  }
  std::vector<ScItem> items(1);
  items[0].img = d_img;
  items[0].stride = stride;
  items[0].W = W;
  items[0].H = H;
  items[0].C = C;
  items[0].tw = tw;
  items[0].th = th;
  items[0].result = 0;
  items[0].opt = opt;
  items[0].padded = true;  // the caller (fi_smartcrop_ex) staged it at a 16-B rounded pitch, + 256 B
  ScLaunchData SL;
  std::vector<int> st(1, FI_OK);
  std::vector<std::string> errs(1);
  plan_smartcrop(c, E, items, &SL, &st, &errs, prescaled != nullptr);
  if (st[0] != FI_OK) return set_err(st[0], "%s", errs[0].c_str());
  *plan_out = *SL.plans[0];
  const size_t results_off = E.work.take(sizeof(ScResult));
  const size_t scores_off = E.work.take(sizeof(CropScore) * std::max(SL.nscores, 1));
  int rc = ensure(c, &c->work, E.work.size + 256);
  if (rc) return rc;
  uint8_t *wb = (uint8_t *)c->work.p;
  ScDesc &d = SL.descs[0];
  fix_ptr(d.red, wb);
  fix_ptr(d.hbuf, wb);
  fix_ptr(d.tbuf, wb);
  fix_ptr(d.pre, wb);
  fix_ptr(d.maps, wb);
  Blob &B = E.blob;
  ScLaunches SX;
  add_sc_launches(c, B, SL, st, &SX);
  const size_t ai_off = B.addv(E.ai), af_off = B.addv(E.af), ad_off = B.addv(E.ad);
  if (!heap_fits(c, E)) return set_err(FI_ENOMEM, "smartcrop tables exceed the device table heap");
  rc = ensure(c, &c->arena, B.b.size() + 256);
  if (rc) return rc;
  rc = ensure_pinned(c, B.b.size() + 256);
  if (rc) return rc;
  memcpy(c->pinned, B.b.data(), B.b.size());
  HIP_TRY(hipMemcpyAsync(c->arena.p, c->pinned, B.b.size(), hipMemcpyHostToDevice, c->stream));
  uint8_t *ab = (uint8_t *)c->arena.p;
  rc = heap_commit(c, E, ab, ai_off, af_off, ad_off);
  if (rc) return rc;
  rc = enqueue_sc(c, c->stream, ab, SX, (const int32_t *)c->heap_i.p, (const double *)c->heap_d.p,
                  (CropScore *)(wb + scores_off), (ScResult *)(wb + results_off), to_dev(params));
  if (rc) return rc;
  scores->resize(SL.nscores);
  HIP_TRY(hipMemcpyAsync(scores->data(), wb + scores_off, sizeof(CropScore) * SL.nscores, hipMemcpyDeviceToHost,
                         c->stream));
  HIP_TRY(hipMemcpyAsync(result, wb + results_off, sizeof(ScResult), hipMemcpyDeviceToHost, c->stream));
  const size_t na = (size_t)d.aw * d.ah;
  if (prescaled) {
    prescaled->resize(na * 3);
    if (d.pre) {
      HIP_TRY(hipMemcpyAsync(prescaled->data(), d.pre, na * 3, hipMemcpyDeviceToHost, c->stream));
    } else {
      // no prescale: the analysed image is the input (C may be 1)
      std::vector<uint8_t> tmp((size_t)stride * H);
      HIP_TRY(hipMemcpyAsync(tmp.data(), d_img, tmp.size(), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
      for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++)
          for (int k = 0; k < 3; k++) (*prescaled)[((size_t)y * W + x) * 3 + k] = tmp[(size_t)y * stride + x * C + (C == 3 ? k : 0)];
    }
  }
  std::vector<uint32_t> pm;
  if (maps) {
    pm.resize(na);
    HIP_TRY(hipMemcpyAsync(pm.data(), d.maps, na * 4, hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  collect_timers(c);
  if (maps) {
    maps->resize(na * 3);
    for (size_t i = 0; i < na; i++) {
      (*maps)[i * 3 + 0] = pm[i] & 255;
      (*maps)[i * 3 + 1] = (pm[i] >> 8) & 255;
      (*maps)[i * 3 + 2] = (pm[i] >> 16) & 255;
    }
  }
  if (result->top < 0) return set_err(FI_EUNSUPPORTED, "smartcrop: scoring kernel rejected the crop count");
  return FI_OK;
}

extern "C" {

// Test hook: the skin / saturation table of k_sc_fz / k_sc_fd for `params`,
// returned in r-major colour order (the device table is in sc_colour_key order)
int fi_debug_skinsat(fi_ctx *c, const fi_smartcrop_params *params, uint16_t *out) {
  if (!c || !out) return set_err(FI_EINVAL, "bad arguments");
  fi_smartcrop_params p;
  if (params)
    p = *params;
  else
    fi_smartcrop_default_params(&p);
  HIP_TRY(hipSetDevice(c->device));
  sync_streams(c);  // batches in flight may read the table
  const int rc = ensure(c, &c->skinsat, (size_t)2 << 24);
  if (rc != FI_OK) return rc;
  const ScParamsDev PD = to_dev(p);
  launch_sc_skinsat(c->stream, (uint16_t *)c->skinsat.p, PD);
  c->skinsat_key.clear();  // built on c->stream, not the smartcrop stream: rebuilt before the next use
  HIP_TRY(hipGetLastError());
  std::vector<uint16_t> z((size_t)1 << 24);
  HIP_TRY(hipMemcpyAsync(z.data(), c->skinsat.p, (size_t)2 << 24, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (uint32_t k = 0; k < (1u << 24); k++) out[k] = z[sc_colour_key(k >> 16, (k >> 8) & 255, k & 255)];  // r-major
  return FI_OK;
}
void fi_smartcrop_default_params(fi_smartcrop_params *p) {
  memset(p, 0, sizeof *p);
  p->detail_weight = 0.2;
  p->edge_radius = 0.4;
  p->edge_weight = -10;
  p->outside_importance = -0.5;
  p->rule_of_thirds = 1;
  p->saturation_bias = 0.2;
  p->saturation_brightness_max = 0.9;
  p->saturation_brightness_min = 0.05;
  p->saturation_threshold = 0.4;
  p->saturation_weight = 0.3;
  p->score_down_sample = 1;
  p->skin_bias = 0.01;
  p->skin_brightness_max = 1;
  p->skin_brightness_min = 0.2;
  p->skin_color[0] = 0.78;
  p->skin_color[1] = 0.57;
  p->skin_color[2] = 0.44;
  p->skin_threshold = 0.8;
  p->skin_weight = 1.8;
}
void fi_smartcrop_default_options(fi_smartcrop_options *o) {
  memset(o, 0, sizeof *o);
  o->prescale = 1;
  o->max_scale = 1;
  o->min_scale = 0.9;
  o->scale_step = 0.1;
  o->step = 8;
  o->exact_all = 0;
}

int fi_smartcrop_ex(fi_ctx *c, const uint8_t *rgb, int32_t w, int32_t h, int32_t stride, int32_t tw, int32_t th,
                    const fi_smartcrop_params *params, const fi_smartcrop_options *opts, fi_crop_score *crops,
                    int32_t crops_cap, int32_t *n_crops, int32_t *top_index, int32_t analyse_wh[2], double *prescale,
                    uint8_t *prescaled_out, uint8_t *maps_out, int64_t out_cap) {
  if (!c || !rgb || w <= 0 || h <= 0 || stride < 3 * w) return set_err(FI_EINVAL, "bad image arguments");
  fi_smartcrop_params P;
  fi_smartcrop_default_params(&P);
  if (params) P = *params;
  if (P.score_down_sample != 1) return set_err(FI_EUNSUPPORTED, "score_down_sample != 1 is not supported");
  fi_smartcrop_options O;
  fi_smartcrop_default_options(&O);
  if (opts) O = *opts;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  int rc = drain(c);  // io / pinned staging are shared with in-flight batches
  if (rc) return rc;
  const int64_t dstride = ((int64_t)w * 3 + 15) / 16 * 16;
  rc = ensure(c, &c->io, (size_t)dstride * h + 256);
  if (rc) return rc;
  HIP_TRY(hipMemcpy2DAsync(c->io.p, dstride, rgb, stride, (size_t)w * 3, h, hipMemcpyHostToDevice, c->stream));
  std::vector<CropScore> scores;
  ScResult res{};
  ScPlan plan;
  std::vector<uint8_t> pre, maps;
  rc = run_smartcrop(c, (const uint8_t *)c->io.p, w, h, dstride, 3, tw, th, P, O, &scores, &res, &plan,
                     prescaled_out ? &pre : nullptr, maps_out ? &maps : nullptr);
  if (rc) return rc;
  const int nc = (int)plan.crops.size();
  if (n_crops) *n_crops = nc;
  if (top_index) *top_index = res.top;
  if (analyse_wh) {
    analyse_wh[0] = plan.aw;
    analyse_wh[1] = plan.ah;
  }
  if (prescale) *prescale = plan.prescale;
  if (crops) {
    for (int k = 0; k < nc && k < crops_cap; k++) {
      const CropHost &ch = plan.crops[k];
      fi_crop_score &o = crops[k];
      o.x = ch.rx;
      o.y = ch.ry;
      o.width = ch.rw;
      o.height = ch.rh;
      o.fx = ch.fx;
      o.fy = ch.fy;
      o.fw = ch.fw;
      o.fh = ch.fh;
      o.detail = scores[k].detail;
      o.saturation = scores[k].saturation;
      o.skin = scores[k].skin;
      o.total = scores[k].total;
      o.exact = scores[k].exact;
      o.pad = 0;
    }
  }
  const size_t na = (size_t)plan.aw * plan.ah * 3;
  if (prescaled_out) {
    if ((int64_t)na > out_cap) return set_err(FI_ECAPACITY, "out_cap < analyse_w*analyse_h*3");
    memcpy(prescaled_out, pre.data(), na);
  }
  if (maps_out) {
    if ((int64_t)na > out_cap) return set_err(FI_ECAPACITY, "out_cap < analyse_w*analyse_h*3");
    memcpy(maps_out, maps.data(), na);
  }
  return FI_OK;
}

int fi_smartcrop(fi_ctx *c, const uint8_t *rgb, int32_t w, int32_t h, int32_t stride, int32_t tw, int32_t th,
                 const fi_smartcrop_params *params, int32_t out_xywh[4], double *out_score) {
  int32_t n = 0, top = -1;
  int32_t awh[2];
  double pre;
  // crops are needed to decode the top index
  std::vector<fi_crop_score> crops(1);
  {
    // first call with a small buffer just to learn the crop count is wasteful;
    // the planner is cheap, so plan here directly
    fi_smartcrop_options O;
    fi_smartcrop_default_options(&O);
    ScPlan p;
    if (plan_sc(w, h, tw, th, O, &p) != FI_OK) return set_err(p.status, "%s", p.err.c_str());
    crops.resize(p.crops.size());
  }
  int rc = fi_smartcrop_ex(c, rgb, w, h, stride, tw, th, params, nullptr, crops.data(), (int32_t)crops.size(), &n,
                           &top, awh, &pre, nullptr, nullptr, 0);
  if (rc) return rc;
  if (top < 0 || top >= n) return set_err(FI_EDEVICE, "smartcrop: no top crop");
  out_xywh[0] = crops[top].x;
  out_xywh[1] = crops[top].y;
  out_xywh[2] = crops[top].width;
  out_xywh[3] = crops[top].height;
  if (out_score) *out_score = crops[top].total;
  return FI_OK;
}

}  // extern "C"
