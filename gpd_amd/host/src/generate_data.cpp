// generate_data CONFIG — the reference's training-set generator CLI (src/generate_data.cpp) on the HIP path: balanced
// (image, label) sets for pytorch/train_net3.py, written as train / test _images.npy and _labels.npy under output_root.
#include <iostream>

#include "gpd/data_generator.h"

int main(int argc, char *argv[]) {
  if (argc < 2) {
    std::cout << "Error: Not enough input arguments!\n\n";
    std::cout << "Usage: generate_data CONFIG_FILE\n\n";
    std::cout << "Generate data using parameters from CONFIG_FILE (*.cfg).\n\n";
    return -1;
  }
  gpd::DataGenerator generator(argv[1]);
  if (!generator.ok()) return -1;
  return generator.generateData() ? 0 : -1;
}
