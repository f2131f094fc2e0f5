// net::Classifier::create and its one back-end, net::HipClassifier — see include/gpd/net/classifier.h (reference:
// net/classifier.cpp, net/eigen_classifier.cpp); candidate::Hand::print (candidate/hand.cpp), the one method of the
// record classes that is not inline.
#include <fstream>
#include <iostream>

#include "gpd/util/config_file.h"
#include "host_internal.h"

namespace gpd {

namespace candidate {
void Hand::print() const {  // hand.cpp:66-79
  auto p = getPosition(), a = getApproach(), b = getBinormal(), x = getAxis();
  printf("position: %g %g %g\napproach: %g %g %g\nbinormal: %g %g %g\naxis: %g %g %g\nscore: %g\n", p[0], p[1], p[2], a[0], a[1],
         a[2], b[0], b[1], b[2], x[0], x[1], x[2], getScore());
  printf("full-antipodal: %d\nhalf-antipodal: %d\nclosing box:\n bottom: %g\n top: %g\n center: %g\n", isFullAntipodal(),
         isHalfAntipodal(), getBottom(), getTop(), getCenter());
}
}  // namespace candidate

namespace net {

// the classifier's own context: created for its channel count, the loaded network installed (installOn)
static bool create_own_context(const HipClassifier &c, gpd_hip_ctx **ctx) {
  gpd_params p;
  gpd_hip_default_params(&p);
  p.image_num_channels = c.channels();
  if (hip_failed(gpd_hip_create(0, &p, ctx))) {
    *ctx = nullptr;
    return false;
  }
  return !hip_failed(c.installOn(*ctx));
}

std::shared_ptr<Classifier> Classifier::create(const std::string &model_file, const std::string &weights_file, Device device,
                                               int batch_size) {
  // one back-end is compiled in, as in the reference's builds (classifier.cpp:46-62); see classifier.h
  if (device != Device::eGPU)
    printf("NOTE: classifier device = %d requested; this build's only back-end (HipClassifier) runs on the GPU.\n", (int)device);
  auto c = std::make_shared<HipClassifier>(model_file, weights_file, device, batch_size);
  if (!c->ok()) return nullptr;
  return c;
}

std::vector<float> HipClassifier::readBinaryFileIntoVector(const std::string &location) {
  std::vector<float> vals;
  std::ifstream file(location.c_str(), std::ios::binary | std::ios::in);
  if (!file.is_open()) {
    std::cout << "ERROR: Cannot open file: " << location << "!\n";
    return vals;
  }
  float x;
  while (file.read(reinterpret_cast<char *>(&x), sizeof(float))) vals.push_back(x);
  return vals;
}

HipClassifier::HipClassifier(const std::string &, const std::string &weights_file, Classifier::Device, int batch_size)
    : batch_size_(batch_size) {
  const std::string &dir = weights_file;
  static const char *files[8] = {"conv1_weights.bin", "conv1_biases.bin", "conv2_weights.bin", "conv2_biases.bin",
                                 "ip1_weights.bin",   "ip1_biases.bin",   "ip2_weights.bin",   "ip2_biases.bin"};
  // A parameter directory describes its own network: network.cfg (written by `python -m gpd_amd.torch_export`) with
  // layout = torch means the eight tensors of the reference's PyTorch network (pytorch/network.py::Net) as torch stores them;
  // they are converted here, once, into the Eigen layouts everything else works with.  No network.cfg: the reference's files.
  static const char *torch_files[8] = {"conv1.weight.bin", "conv1.bias.bin", "conv2.weight.bin", "conv2.bias.bin",
                                       "fc1.weight.bin",   "fc1.bias.bin",   "fc2.weight.bin",   "fc2.bias.bin"};
  bool torch_layout = false;
  double input_scale = 1.0;
  int net_shape[4] = {-1, -1, -1, -1};  // conv1_out, conv2_out, fc1_out, fc2_out of network.cfg, when it has them
  if (std::ifstream((dir + "network.cfg").c_str()).good()) {
    util::ConfigFile net_cfg(dir + "network.cfg");
    net_cfg.ExtractKeys();
    const std::string layout = net_cfg.getValueOfKeyAsString("layout", "eigen");
    if (layout != "torch" && layout != "eigen") {
      printf("ERROR: %snetwork.cfg: unknown layout '%s' (torch or eigen)\n", dir.c_str(), layout.c_str());
      return;
    }
    torch_layout = layout == "torch";
    const int relu = net_cfg.getValueOfKey<int>("conv_relu", torch_layout ? 1 : 0);
    if (relu != 0 && relu != 1) {
      printf("ERROR: %snetwork.cfg: conv_relu = %d (0 or 1)\n", dir.c_str(), relu);
      return;
    }
    conv_relu_ = relu != 0;
    input_scale = net_cfg.getValueOfKey<double>("input_scale", torch_layout ? 1.0 / 256 : 1.0);
    if (!torch_layout && input_scale != 1.0) {
      printf("ERROR: %snetwork.cfg: input_scale needs layout = torch\n", dir.c_str());
      return;
    }
    static const char *shape_keys[4] = {"conv1_out", "conv2_out", "fc1_out", "fc2_out"};
    for (int i = 0; i < 4; i++) net_shape[i] = net_cfg.getValueOfKey<int>(shape_keys[i], -1);
  }
  // network.cfg with conv1_out / conv2_out / fc1_out [/ fc2_out]: another member of the reference's network family
  // (pytorch/network.py: other widths, NetCCFFF), which the shape-general route scores (gpd_hip_set_lenet_net)
  if (net_shape[0] != -1 || net_shape[1] != -1 || net_shape[2] != -1 || net_shape[3] != -1) {
    if (!torch_layout) {
      printf("ERROR: %snetwork.cfg: conv1_out / conv2_out / fc1_out / fc2_out need layout = torch\n", dir.c_str());
      return;
    }
    loadGeneral(dir, net_shape, input_scale);
    return;
  }
  for (int i = 0; i < 8; i++) params_[i] = readBinaryFileIntoVector(dir + (torch_layout ? torch_files[i] : files[i]));
  const auto &c1w = params_[0];
  if (c1w.size() % 500 != 0 || c1w.empty() || params_[1].size() != 20 || params_[2].size() != 25000 || params_[3].size() != 50 ||
      params_[4].size() != 3600000 || params_[5].size() != 500 || params_[6].size() != 1000 || params_[7].size() != 2) {
    printf("ERROR: LeNet parameter files in %s are missing or have unexpected sizes\n", dir.c_str());
    return;
  }
  if (torch_layout) {
    // conv2 and the biases are the same in both layouts (gpd_hip.h, gpd_hip_lenet_from_torch)
    std::vector<float> c1(params_[0].size()), f1(params_[4].size()), f2(params_[6].size());
    if (gpd_hip_lenet_from_torch((int)(c1w.size() / 500), input_scale, params_[0].data(), params_[4].data(), params_[6].data(), c1.data(),
                                 f1.data(), f2.data()) != GPD_OK) {
      printf("ERROR: %snetwork.cfg: %s\n", dir.c_str(), gpd_hip_last_error());
      return;
    }
    params_[0].swap(c1);
    params_[4].swap(f1);
    params_[6].swap(f2);
  }
  channels_ = (int)(c1w.size() / 500);
  loaded_ = create_own_context(*this, &ctx_);
}

// A torch directory of another shape: the 8 (Net) or 10 (NetCCFFF) tensors as torch stores them, converted once by
// gpd_hip_lenet_net_from_torch into the general route's layouts (net_), and installed in the classifier's own context.
void HipClassifier::loadGeneral(const std::string &dir, const int widths[4], double input_scale) {
  static const char *names[10] = {"conv1.weight.bin", "conv1.bias.bin", "conv2.weight.bin", "conv2.bias.bin", "fc1.weight.bin",
                                  "fc1.bias.bin",     "fc2.weight.bin", "fc2.bias.bin",   "fc3.weight.bin", "fc3.bias.bin"};
  const int F1 = widths[0], F2 = widths[1], H1 = widths[2], H2 = widths[3] == -1 ? 0 : widths[3];
  const int files = H2 > 0 ? 10 : 8;
  std::vector<float> raw[10];
  for (int i = 0; i < files; i++) raw[i] = readBinaryFileIntoVector(dir + names[i]);
  const size_t per_channel = F1 > 0 ? (size_t)F1 * 25 : 1;
  shape_ = {(int32_t)(raw[0].size() / per_channel), F1, F2, H1, H2};
  if (gpd_hip_lenet_shape_check(&shape_) != GPD_OK) {
    printf("ERROR: %snetwork.cfg: %s\n", dir.c_str(), gpd_hip_last_error());
    return;
  }
  const size_t N = H2 > 0 ? (size_t)H2 : 2;
  const size_t want[10] = {(size_t)F1 * shape_.channels * 25, (size_t)F1, (size_t)F2 * F1 * 25, (size_t)F2, (size_t)H1 * F2 * 144, (size_t)H1,
                           N * H1, N, (size_t)2 * H2, (size_t)(H2 > 0 ? 2 : 0)};
  for (int i = 0; i < files; i++)
    if (raw[i].size() != want[i]) {
      printf("ERROR: LeNet parameter files in %s are missing or have unexpected sizes\n", dir.c_str());
      return;
    }
  const float *in[10];
  float *out[10];
  for (int i = 0; i < 10; i++) {
    net_[i].assign(i < files ? want[i] : 0, 0.f);
    in[i] = i < files ? raw[i].data() : nullptr;
    out[i] = i < files ? net_[i].data() : nullptr;
  }
  if (gpd_hip_lenet_net_from_torch(&shape_, input_scale, in, out) != GPD_OK) {
    printf("ERROR: %snetwork.cfg: %s\n", dir.c_str(), gpd_hip_last_error());
    return;
  }
  general_ = true;
  channels_ = shape_.channels;
  loaded_ = create_own_context(*this, &ctx_);
}

int HipClassifier::installOn(gpd_hip_ctx *ctx) const {
  int rc;
  if (general_) {
    const float *t[10];
    for (int i = 0; i < 10; i++) t[i] = net_[i].empty() ? nullptr : net_[i].data();
    rc = gpd_hip_set_lenet_net(ctx, &shape_, t);
  } else {
    rc = gpd_hip_set_lenet_weights(ctx, channels_, params_[0].data(), params_[1].data(), params_[2].data(), params_[3].data(), params_[4].data(),
                                   params_[5].data(), params_[6].data(), params_[7].data());
  }
  return rc != GPD_OK ? rc : gpd_hip_set_lenet_conv_relu(ctx, conv_relu_ ? 1 : 0);
}

HipClassifier::~HipClassifier() {
  if (ctx_) gpd_hip_destroy(ctx_);
}

// one of the two arithmetic switches of a loaded classifier's own context
static bool set_mode(const HipClassifier &c, gpd_hip_ctx *ctx, int (*setter)(gpd_hip_ctx *, int), int mode) {
  return c.ok() && !hip_failed(setter(ctx, mode));
}

bool HipClassifier::setScoringMode(int mode) { return set_mode(*this, ctx_, gpd_hip_set_lenet_mode, mode); }

bool HipClassifier::setNetMode(int mode) { return set_mode(*this, ctx_, gpd_hip_set_lenet_net_mode, mode); }

std::vector<float> HipClassifier::classifyImages(const std::vector<std::unique_ptr<Image>> &image_list) {
  std::vector<float> out(image_list.size(), 0.f);
  if (!ok()) return out;
  const size_t bytes = (size_t)60 * 60 * channels_;
  std::vector<uint8_t> batch;
  std::vector<size_t> where;
  batch.reserve(image_list.size() * bytes);
  for (size_t i = 0; i < image_list.size(); i++) {
    const Image &im = *image_list[i];
    // non-continuous images are skipped and keep score 0 (eigen_classifier.cpp:68)
    if (!im.isContinuous() || im.rows != 60 || im.cols != 60 || im.channels() != channels_ || im.data.size() != bytes) continue;
    batch.insert(batch.end(), im.data.begin(), im.data.end());
    where.push_back(i);
  }
  std::vector<float> s(where.size());
  if (!where.empty() && hip_failed(gpd_hip_score(ctx_, batch.data(), (int)where.size(), s.data()))) return out;
  for (size_t k = 0; k < where.size(); k++) out[where[k]] = s[k];
  return out;
}

}  // namespace net
}  // namespace gpd
