// net::Classifier — the reference's plugin surface (net/classifier.h:52-81) with a HIP back-end.
// cv::Mat is absent here; `Image` carries what classifyImages reads from it (rows, cols,
// channels, data pointer, continuity; eigen_classifier.cpp:64-74, 130-149).
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

struct gpd_hip_ctx;

namespace gpd {
namespace net {

struct Image {  // stand-in for cv::Mat CV_8UC(C), HWC interleaved
  int rows = 0, cols = 0, channels_ = 0;
  std::vector<uint8_t> data;
  bool continuous = true;
  Image() {}
  Image(int r, int c, int ch) : rows(r), cols(c), channels_(ch), data((size_t)r * c * ch, 0) {}
  bool isContinuous() const { return continuous; }
  int channels() const { return channels_; }
};

class Classifier {
 public:
  enum class Device : uint8_t { eCPU = 0, eGPU = 1, eVPU = 2, eFPGA = 3 };
  virtual ~Classifier() {}
  // The reference's factory (classifier.cpp:46-62) picks its back-end at COMPILE time (USE_OPENVINO / USE_CAFFE /
  // Eigen) and only hands `device` on to it; the Eigen back-end ignores it altogether
  // (eigen_classifier.cpp:6-9).  This build is compiled with exactly one back-end, HipClassifier, so — like the
  // reference's Eigen build — every `device` value yields that back-end: a reference cfg without a `device` key
  // (-> 0 = eCPU, grasp_detector.cpp:133) gets the HIP classifier too.  There is no CPU path behind the
  // interface; a value other than eGPU is reported once on stdout, nothing else changes.
  // weights_file: the parameter directory ending in '/', as for EigenClassifier (eigen_classifier.cpp:28-50);
  // model_file and batch_size are accepted and unused, as there.  nullptr when the parameters cannot be loaded.
  static std::shared_ptr<Classifier> create(const std::string &model_file, const std::string &weights_file,
                                            Device device = Device::eCPU, int batch_size = 1);
  virtual std::vector<float> classifyImages(const std::vector<std::unique_ptr<Image>> &image_list) = 0;
  virtual int getBatchSize() const = 0;
};

class HipClassifier : public Classifier {
 public:
  HipClassifier(const std::string &model_file, const std::string &weights_file, Classifier::Device device, int batch_size);
  ~HipClassifier() override;
  std::vector<float> classifyImages(const std::vector<std::unique_ptr<Image>> &image_list) override;
  int getBatchSize() const override { return batch_size_; }
  bool ok() const { return ctx_ != nullptr && loaded_; }
  // Arithmetic of the scoring kernels (gpd_hip_set_lenet_mode): 0 = operands split exactly over the int8 / bf16 matrix
  // pipes (default: within 1e-4 of EigenClassifier's plain-float result, closer to float64 than it), 1 = the f32 chain
  // in the reference's own operation order.  GraspDetector sets it from the cfg key `hip_lenet_mode`.
  bool setScoringMode(int mode);
  // Arithmetic of the shape-general route (gpd_hip_set_lenet_net_mode): 0 = the f32 chains (default), 1 = split operands on
  // the bf16 matrix pipe.  GraspDetector sets it from the cfg key `hip_lenet_net_mode`.
  bool setNetMode(int mode);
  // raw float32 parameter file -> vector (EigenClassifier::readBinaryFileIntoVector, :185-204)
  static std::vector<float> readBinaryFileIntoVector(const std::string &location);
  // The parameters as read from the files (conv1 w, b, conv2 w, b, ip1 w, b, ip2 w, b): GraspDetector loads the
  // same arrays into the context of its fused search -> image -> score path.
  int channels() const { return channels_; }
  // The parameter directory may hold a network.cfg (python -m gpd_amd.torch_export writes one): layout = torch — the files
  // are conv1.weight.bin ... fc2.bias.bin of the reference's PyTorch network (pytorch/network.py::Net) in torch layout,
  // converted on load by gpd_hip_lenet_from_torch with input_scale folded into conv1, so parameter(i) below is in the Eigen
  // layouts either way; conv_relu = 1 — a ReLU after conv1 and conv2 (gpd_hip_set_lenet_conv_relu), which GraspDetector sets
  // on the fused path's context as well.  Without the file: the reference's Eigen network, as ever.
  bool convRelu() const { return conv_relu_; }
  const std::vector<float> &parameter(int i) const { return params_[i]; }
  // A network.cfg that also names conv1_out, conv2_out, fc1_out [and fc2_out > 0: NetCCFFF, with fc3.weight.bin / fc3.bias.bin]
  // describes another member of the reference's network family; it is loaded through gpd_hip_lenet_net_from_torch and
  // scored on the shape-general route (gpd_hip_set_lenet_net).  parameter(i) is empty then.
  bool general() const { return general_; }
  const gpd_lenet_shape &shape() const { return shape_; }
  // The loaded network and its conv ReLU flag into a context (the classifier's own, and GraspDetector's fused path's):
  // gpd_hip_set_lenet_weights or gpd_hip_set_lenet_net, then gpd_hip_set_lenet_conv_relu -> GPD_OK or the first error
  int installOn(gpd_hip_ctx *ctx) const;

 private:
  gpd_hip_ctx *ctx_ = nullptr;
  bool loaded_ = false;
  int channels_ = 0;
  bool conv_relu_ = false;
  int batch_size_ = 1;
  std::vector<float> params_[8];
  void loadGeneral(const std::string &dir, const int widths[4], double input_scale);
  bool general_ = false;
  gpd_lenet_shape shape_ = {0, 0, 0, 0, 0};
  std::vector<float> net_[10];  // the general route's layouts
};

}  // namespace net
}  // namespace gpd
