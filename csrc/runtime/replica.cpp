// Inference replicas (see replica.h).
#include "replica.h"

#include <math.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <stdexcept>

#include "../codec/json_codec.h"

namespace gale {

// ---------------------------------------------------------------------------------------------
// StubReplica
// ---------------------------------------------------------------------------------------------

StubReplica::StubReplica(int H, int W, int C, int classes, int max_images, int delay_us,
                         bool compute, int locality)
    : H_(H), W_(W), C_(C), classes_(classes), max_images_(max_images), delay_us_(delay_us),
      compute_(compute), locality_(locality) {
  x_.resize((size_t)max_images * H * W * C);
  probs_.resize((size_t)max_images * classes);
}

void StubReplica::set_input_resize(const InputResize& r) {
  if (r.H() != H_ || r.W() != W_ || !r.ok())
    throw std::invalid_argument("StubReplica: resize tables do not match the model input");
  resize_ = r;
  src_.resize((size_t)max_images_ * r.HS() * r.WS() * C_);
}

void StubReplica::submit(Batch& b) {
  const size_t per = (size_t)H_ * W_ * C_;
  // the size the records' images arrive in, and where they are parsed
  const int RH = resize_ ? resize_->HS() : H_;
  const int RW = resize_ ? resize_->WS() : W_;
  const size_t rper = (size_t)RH * RW * C_;
  float* const parsed = resize_ ? src_.data() : x_.data();
  int slot = 0;
  b.dev_status.assign(b.recs.size(), codec::OK);
  if (!compute_) {
    int n = 0;
    for (const InRecord& r : b.recs) n += r.images;
    std::fill(probs_.begin(), probs_.begin() + (size_t)n * classes_, 1.0f / (float)classes_);
    if (delay_us_ > 0) usleep((useconds_t)delay_us_);
    b.probs = probs_.data();
    b.pred_text = nullptr;
    return;
  }
  for (size_t ri = 0; ri < b.recs.size(); ++ri) {
    InRecord& r = b.recs[ri];
    int n = 0;
    // an NCHW record is a rectangular array of dims (C, H, W) to the dims-agnostic decoder
    const bool nchw = prep_.nchw != 0;
    // (a b64 string's bytes are in record order too: [C][H][W] with nchw)
    const int st = b64_ ? pixels_.parse_host(r.value, (size_t)r.len, RH, RW, C_,
                                             parsed + (size_t)slot * rper, max_images_ - slot,
                                             &n)
                        : codec::parse_instances_host(r.value, (size_t)r.len, nchw ? C_ : RH,
                                                      nchw ? RH : RW, nchw ? RW : C_,
                                                      parsed + (size_t)slot * rper,
                                                      max_images_ - slot, &n);
    if (st != codec::OK) b.dev_status[ri] = st;
    else if (!prep_.identity())
      codec::apply_input_prep(parsed + (size_t)slot * rper, n, RH, RW, C_, nchw, prep_.a,
                              prep_.b);
    if (resize_ && st == codec::OK) {
      resize_->apply_host(src_.data() + (size_t)slot * rper, n, C_,
                          x_.data() + (size_t)slot * per);
      resized_ += n;
    }
    for (int i = 0; i < r.images; ++i) {
      const float* img = x_.data() + (size_t)(slot + i) * per;
      float* out = probs_.data() + (size_t)(slot + i) * classes_;
      if (st != codec::OK) {
        std::fill(out, out + classes_, 0.f);
        continue;
      }
      double mx = -1e300;
      for (int k = 0; k < classes_; ++k) {
        double s = 0;
        for (size_t p = (size_t)(k % C_); p < per; p += (size_t)C_) s += img[p];
        const double logit = (k + 1) * s / (double)(per / (size_t)C_);
        out[k] = (float)logit;
        mx = std::max(mx, logit);
      }
      double sum = 0;
      for (int k = 0; k < classes_; ++k) sum += exp((double)out[k] - mx);
      for (int k = 0; k < classes_; ++k) out[k] = (float)(exp((double)out[k] - mx) / sum);
    }
    slot += r.images;
  }
  if (delay_us_ > 0) usleep((useconds_t)delay_us_);
  b.probs = probs_.data();
  b.pred_text = nullptr;
}

void StubReplica::wait(Batch& b) { (void)b; }

}  // namespace gale
