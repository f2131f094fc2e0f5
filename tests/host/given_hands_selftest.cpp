// given_hands_selftest CONFIG PCD PCD2 OUT_PREFIX — hand sets found by one gpd::GraspDetector on one cloud, imaged and pruned by
// ANOTHER detector over a modified cloud (run by tests/test_gpu_given_hands_host.py on the GPU):
//   GraspDetector::createImages and pruneGraspCandidates with hand sets that are not the last search's go through
//   gpd_hip_images_given / gpd_hip_score_given — no second search, and no "not the last generateGraspCandidates call" error.
// Written for the test to compare with the Python route, all raw:
//   OUT_PREFIX.given    the hand sets handed over, [sets][slots] gpd_hand records (set_index as listed, valid as filtered)
//   OUT_PREFIX.images   createImages' images, [n][60][60][C] u8
//   OUT_PREFIX.hands    createImages' hands, [n] records
//   OUT_PREFIX.pruned   pruneGraspCandidates' hands (min_score -1e30: all of them), [n] records with scores
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "gpd/grasp_detector.h"

static int fail(const char *what) {
  printf("SELFTEST FAILED: %s\n", what);
  return 1;
}

static bool dump(const std::string &path, const void *data, size_t bytes) {
  FILE *f = fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = bytes == 0 || fwrite(data, 1, bytes, f) == bytes;
  return fclose(f) == 0 && ok;
}

int main(int argc, char *argv[]) {
  if (argc < 5) return fail("usage: given_hands_selftest CONFIG PCD PCD2 OUT_PREFIX");
  const std::string prefix = argv[4];
  gpd::util::Cloud cloud(argv[2], {0.0, 0.0, 0.0}), other(argv[3], {0.0, 0.0, 0.0});
  gpd::GraspDetector finder(argv[1]);
  if (!finder.ok() || cloud.size() == 0 || other.size() == 0) return fail("setup");
  finder.preprocessPointCloud(cloud);
  auto sets = finder.generateGraspCandidates(cloud);
  const std::vector<double> ws = {-1, 1, -1, 1, -1, 1};
  auto filtered = finder.filterGraspsWorkspace(sets, ws);
  if (filtered.empty()) return fail("no hand sets");
  const size_t slots = filtered[0]->getHands().size();
  std::vector<gpd_hand> given;
  for (size_t s = 0; s < filtered.size(); s++) {
    if (filtered[s]->getHands().size() != slots) return fail("hand sets of different sizes");
    for (size_t j = 0; j < slots; j++) {
      gpd_hand r = filtered[s]->getHands()[j]->record();
      r.set_index = (int)s;
      r.valid = filtered[s]->getIsValid()[j] ? 1 : 0;
      given.push_back(r);
    }
  }
  // another detector, which has searched nothing, over the modified cloud
  gpd::GraspDetector user(argv[1]);
  if (!user.ok()) return fail("second detector");
  user.preprocessPointCloud(other);
  std::vector<std::unique_ptr<gpd::net::Image>> images;
  std::vector<std::unique_ptr<gpd::candidate::Hand>> hands;
  if (!user.createImages(other, filtered, images, hands)) return fail("createImages refused hand sets of another detector");
  if (images.empty() || images.size() != hands.size()) return fail("createImages count");
  std::vector<uint8_t> pix;
  std::vector<gpd_hand> recs;
  for (size_t i = 0; i < images.size(); i++) {
    pix.insert(pix.end(), images[i]->data.begin(), images[i]->data.end());
    recs.push_back(hands[i]->record());
  }
  auto pruned = user.pruneGraspCandidates(other, filtered, -1e30);
  if (pruned.size() != hands.size()) return fail("pruneGraspCandidates count");
  std::vector<gpd_hand> prec;
  for (auto &h : pruned) prec.push_back(h->record());
  // ... and a second time, after the detector has searched its own cloud in between: the route does not depend on what is resident
  auto own = user.generateGraspCandidates(other);
  auto again = user.pruneGraspCandidates(other, filtered, -1e30);
  if (again.size() != pruned.size()) return fail("second pruneGraspCandidates count");
  for (size_t i = 0; i < again.size(); i++)
    if (std::memcmp(&again[i]->record(), &prec[i], sizeof(gpd_hand)) != 0) return fail("second pruneGraspCandidates differs");
  if (!dump(prefix + ".given", given.data(), given.size() * sizeof(gpd_hand)) || !dump(prefix + ".images", pix.data(), pix.size()) ||
      !dump(prefix + ".hands", recs.data(), recs.size() * sizeof(gpd_hand)) ||
      !dump(prefix + ".pruned", prec.data(), prec.size() * sizeof(gpd_hand)))
    return fail("writing the dumps");
  printf("SELFTEST OK: %zu hand sets of %zu slots, %zu candidates imaged and pruned on the other cloud\n", filtered.size(), slots,
         images.size());
  return 0;
}
