// Host planner driver (tests/test_plan_digest_cpu.py, tests/test_sanitize_cpu.py):
// reads one image per stdin line
//   W H C target_w target_h flags gravity rotate smartcrop_w smartcrop_h
// and runs everything fi_plan.h declares for it -- plan_im with its shear
// plan, both tap axes, the quantised weights, the MFMA tables of the three
// resample kernels, the smartcrop plan with its Pillow and fragment tables,
// the importance tables and the score fragments -- printing per builder
//   <line> <builder> <64-bit FNV-1a of every scalar field and vector | refused>
// and a closing DONE line with, per builder, how many inputs it built and how
// many it refused, and how often each table variant was reached (a second
// k-step, an uneven row list, a partial last block, ...).  It uses only
// fi_plan.h, so the same file compiles against any split of the planner.
// Built with -fsanitize=address,undefined (host only) by the sanitizer test:
// any out-of-bounds access, overflow or UB in the planner aborts the run.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

#include "../../flyimg_amd/csrc/fi_plan.h"

using namespace fi;

struct Fnv {
  uint64_t h = 1469598103934665603ull;
  void bytes(const void *p, size_t n) {
    const uint8_t *b = static_cast<const uint8_t *>(p);
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
  }
  template <class T>
  Fnv &operator<<(const T &v) {  // one scalar field (never a whole struct: no padding bytes)
    static_assert(std::is_arithmetic<T>::value, "scalars only");
    bytes(&v, sizeof v);
    return *this;
  }
  Fnv &operator<<(const std::string &s) {
    *this << (uint64_t)s.size();
    bytes(s.data(), s.size());
    return *this;
  }
  template <class T>
  Fnv &operator<<(const std::vector<T> &v) {
    static_assert(std::is_arithmetic<T>::value, "vectors of scalars only");
    *this << (uint64_t)v.size();
    bytes(v.data(), v.size() * sizeof(T));
    return *this;
  }
};

static int g_line = 0;
static std::vector<std::string> g_order;                // builders and variants in first-seen order
static std::map<std::string, std::pair<int, int>> g_n;  // built, refused
static std::pair<int, int> &counter(const char *name) {
  if (!g_n.count(name)) g_order.push_back(name);
  return g_n[name];
}
static void emit(const char *name, bool built, const Fnv &f) {
  auto &c = counter(name);
  if (built) {
    c.first++;
    printf("%d %s %016llx\n", g_line, name, (unsigned long long)f.h);
  } else {
    c.second++;
    printf("%d %s refused\n", g_line, name);
  }
}
// a table variant reached by this input (counted in DONE as name=count)
static void reached(const char *name, bool yes) { counter(name).first += yes ? 1 : 0; }

static void hash_shear(Fnv &f, const ShearPlan &s) {
  f << s.on << s.rot << s.sx << s.sy << s.w << s.h << s.bx << s.by << s.cols << s.rows;
  for (const RotShear &q : s.sh) f << q.s << q.width << q.height << q.x_off << q.y_off;
  f << s.cx << s.cy << s.cw << s.ch << s.contained;
}
static void hash_axis(Fnv &f, const AxisTable &t) {
  f << t.start << t.count << t.woff << t.w << t.wd << t.maxtaps << t.src_lo << t.src_hi << t.touched;
}

static void run_axis_tables(const AxisTable &v, const AxisTable &h) {
  for (int ax = 0; ax < 2; ax++) {
    const AxisTable &t = ax ? h : v;
    std::vector<int32_t> wq, q22;
    const int s = vr_quant(t, &wq);
    Fnv a;
    a << s << wq;
    emit(ax ? "vr_quant_h" : "vr_quant_v", s > 0, a);
    Fnv b;
    b << axis_q22(t, &q22) << q22;
    emit(ax ? "axis_q22_h" : "axis_q22_v", true, b);
  }
  reached("axis.outputs_not_16n", v.start.size() % 16 != 0 && h.start.size() % 16 != 0);
  for (int mx : {168, 64, 48, 32}) {
    MfmaH m;
    const bool ok = build_mfma_h(h, &m, mx);
    Fnv f;
    f << m.cols << (uint64_t)m.strips.size();
    bool ks2 = false;
    for (const MfmaStrip &S : m.strips) {
      f << S.x0 << S.x1 << S.b0 << S.nbytes << S.c_lo << S.ncols << S.pitch << S.vpitch << S.nocb << S.ks
        << S.lut_px0 << S.lut_n << (uint64_t)S.frag << (uint64_t)S.s0 << (uint64_t)S.lut << (uint64_t)S.frag2;
      ks2 = ks2 || S.ks == 2;
    }
    f << m.frag << m.s0 << m.lut << m.wsum << m.shift2 << m.frag2 << m.wsum2;
    const std::string name = "mfma_h" + std::to_string(mx);
    emit(name.c_str(), ok, f);
    reached("mfma_h.frag2", ok && !m.frag2.empty());
    reached("mfma_h.ks2", ok && ks2);
    reached("mfma_h.frag2_ks2", ok && ks2 && !m.frag2.empty());
  }
  {
    VmV m;
    const bool ok = build_vm_v(v, &m);
    Fnv f;
    f << m.rows << m.nblk << m.plo << m.pn << m.pblk << m.plast << m.frag << m.w128 << m.row0 << m.rstep;
    emit("vm_v", ok, f);
    reached("vm_v.rstep0", ok && m.rstep == 0);
  }
  {
    VrV m;
    const bool ok = build_vr_v(v, &m);
    Fnv f;
    f << m.rows << m.row0 << m.rstep << m.nblk << m.shift << m.bmeta << m.frag << m.w128 << m.maxgap;
    emit("vr_v", ok, f);
    bool ks2 = false;
    for (size_t b = 0; ok && 4 * b + 1 < m.bmeta.size(); b++) ks2 = ks2 || m.bmeta[4 * b + 1] == 2;
    reached("vr_v.ks2", ok && ks2);
    reached("vr_v.rstep0", ok && m.rstep == 0);
  }
  {
    HvH m;
    const bool ok = build_hv_h(h, &m);
    Fnv f;
    f << m.col0 << (uint64_t)m.strips.size();
    for (const HvStrip &S : m.strips) f << S.x0 << S.x1 << S.px0 << S.pp << S.nocb << (uint64_t)S.frag << (uint64_t)S.s0;
    f << m.frag << m.s0 << m.w128;
    emit("hv_h", ok, f);
    bool ks2 = false;
    for (size_t b = 0; ok && 2 * b + 1 < m.s0.size(); b++) ks2 = ks2 || m.s0[2 * b + 1] == 2;
    reached("hv_h.ks2", ok && ks2);
  }
  {
    HvV m;
    const bool ok = build_hv_v(v, &m);
    Fnv f;
    f << m.row0 << m.nrows << m.nblk << m.k0ks << m.frag << m.wsum;
    emit("hv_v", ok, f);
    bool ks2 = false;
    for (size_t b = 0; ok && 2 * b + 1 < m.k0ks.size(); b++) ks2 = ks2 || m.k0ks[2 * b + 1] == 2;
    reached("hv_v.ks2", ok && ks2);
  }
}

static void run_smartcrop(int W, int H, int scw, int sch) {
  fi_smartcrop_options o{};
  o.prescale = 1;
  o.max_scale = 1;
  o.min_scale = 0.9;
  o.scale_step = 0.1;
  o.step = 8;
  o.exact_all = 1;
  ScPlan p;
  const int rc = plan_sc(W, H, scw > 0 ? scw : 100, sch > 0 ? sch : 100, o, &p);
  if (rc == FI_OK) plan_sc_prep(&p);  // (plan_sc ran it already: it must be repeatable)
  Fnv f;
  f << p.status << p.err << p.W << p.H << p.prescale << p.cw << p.ch << p.thumb << p.fx << p.fy << p.rw << p.rh
    << p.aw << p.ah << p.need_h << p.need_v << p.ksh << p.ksv << p.ybox_first << p.hrows << p.hb << p.hk << p.vb
    << p.vk << p.hkT << p.prep_ok << p.h_chunks << p.h_lds << p.v_chunks << p.v_lds << p.hm_ok << p.hm_ks
    << p.hm_pitch << p.hm_rows << p.hm_nb << p.hm_lds << p.hm_chunks << p.hmB << p.hmC << p.hmS0 << p.vq_ok
    << p.vq_chunks << p.vq_lds << p.cx_ok << p.cx_kv << p.cx_tp << p.cxA << p.cxK0 << p.fz_ok << p.fz_lds << p.vqA
    << p.vqC << p.vqK0 << (uint64_t)p.crops.size();
  for (const CropHost &c : p.crops)
    f << c.fx << c.fy << c.fw << c.fh << c.x0 << c.y0 << c.nin_x << c.nin_y << c.rx << c.ry << c.rw << c.rh;
  emit("plan_sc", rc == FI_OK, f);
  if (rc != FI_OK) return;
  reached("sc.hm", p.hm_ok);
  reached("sc.hm_ks2", p.hm_ok && p.hm_ks == 2);
  reached("sc.vq", p.vq_ok);
  reached("sc.cx", p.cx_ok);
  reached("sc.cx_kv2", p.cx_ok && p.cx_kv == 2);
  reached("sc.fz", p.fz_ok);
  reached("sc.reduce", p.fx > 1 || p.fy > 1);
  reached("sc.hm_not_vq", p.hm_ok && !p.vq_ok);
  fi_smartcrop_params prm{};
  prm.detail_weight = 0.2;
  prm.edge_radius = 0.4;
  prm.edge_weight = -10;
  prm.outside_importance = -0.5;
  prm.rule_of_thirds = 1;
  prm.score_down_sample = 1;
  const CropHost &c0 = p.crops[0];
  std::vector<double> whole, win;
  sc_importance_table(prm, c0.fw, c0.fh, p.aw, p.ah, &whole);
  Fnv a;
  a << whole;
  emit("importance_image", true, a);
  // the table of the first crop's window, as the batch planner sizes it
  const int nx = std::max(c0.nin_x, 1), ny = std::max(c0.nin_y, 1);
  sc_importance_table(prm, c0.fw, c0.fh, nx, ny, &win);
  Fnv b;
  b << nx << ny << win;
  emit("importance_window", true, b);
  reached("importance.wider_than_64", nx > 64);
  for (int nslot = 1; nslot <= kSgSlots; nslot++) {
    ScoreBTab t;
    sc_score_btab(win, nx, ny, prm.outside_importance, nslot, o.step, &t);
    Fnv s;
    s << t.ok << t.q << t.nrows << t.ks;
    for (int32_t d : t.S) s << d;
    s << t.frag;
    const std::string name = "score_btab" + std::to_string(nslot);
    emit(name.c_str(), t.ok, s);
    reached("score_btab.ks1", t.ok && t.ks == 1);
    reached("score_btab.ks2", t.ok && t.ks == 2);
  }
  {  // the whole analysed image as one window: past kSgMaxKs k-steps it refuses
    ScoreBTab t;
    sc_score_btab(whole, p.aw, p.ah, prm.outside_importance, 1, o.step, &t);
    Fnv s;
    s << t.ok << t.q << t.nrows << t.ks;
    for (int32_t d : t.S) s << d;
    s << t.frag;
    emit("score_btab_image", t.ok, s);
  }
}

int main() {
  int W, H, C, tw, th, rot, scw, sch, grav;
  unsigned flags;
  while (scanf("%d %d %d %d %d %u %d %d %d %d", &W, &H, &C, &tw, &th, &flags, &grav, &rot, &scw, &sch) == 10) {
    fi_image im{};
    im.src_w = W;
    im.src_h = H;
    im.src_channels = C;
    im.src_stride = W * C;
    im.target_w = tw;
    im.target_h = th;
    im.flags = flags;
    im.gravity = grav;
    im.rotate = rot;
    ImPlan p;
    const int rc = plan_im(im, &p);
    g_line++;
    Fnv f;
    f << p.status << p.err << p.W << p.H << p.C << p.tw << p.th << p.resize << p.sample << p.sw << p.sh << p.filter
      << p.hfirst << p.xf << p.yf << p.ex0 << p.ey0 << p.ew << p.eh << p.gray << p.mono << p.rot << p.out_w
      << p.out_h << p.out_c << p.conv;
    for (double v : p.cv) f << v;
    hash_shear(f, p.shear);
    f << p.iw << p.ih << p.bg;
    emit("plan_im", rc == FI_OK, f);
    if (rc != FI_OK) continue;
    reached("plan_im.gray", p.gray);
    reached("plan_im.shear", p.shear.on);
    if (p.resize) {
      AxisTable v, h;
      build_axis(p.filter, p.yf, p.sh, p.th, p.ey0, p.ey0 + p.eh, p.sample, p.H, &v);
      build_axis(p.filter, p.xf, p.sw, p.tw, p.ex0, p.ex0 + p.ew, p.sample, p.W, &h);
      Fnv fv, fh;
      hash_axis(fv, v);
      hash_axis(fh, h);
      emit("axis_v", true, fv);
      emit("axis_h", true, fh);
      run_axis_tables(v, h);
    }
    if (flags & FI_OP_SMARTCROP) run_smartcrop(p.out_w, p.out_h, scw, sch);
  }
  printf("DONE %d images;", g_line);
  for (const std::string &k : g_order) {
    const auto &c = g_n[k];
    if (k.find('.') == std::string::npos)
      printf(" %s=%d/%d", k.c_str(), c.first, c.second);
    else
      printf(" %s=%d", k.c_str(), c.first);
  }
  printf("\n");
  return 0;
}
