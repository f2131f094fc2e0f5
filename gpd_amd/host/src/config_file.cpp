// util::ConfigFile — see include/gpd/util/config_file.h (reference: util/config_file.cpp).  Plain C++: nothing of
// libgpd_hip.so is called here.
#include "gpd/util/config_file.h"

#include <fstream>
#include <iostream>

namespace gpd {
namespace util {

static std::string trim(const std::string &s) {
  const char *ws = " \t\r\n";
  size_t a = s.find_first_not_of(ws);
  if (a == std::string::npos) return "";
  size_t b = s.find_last_not_of(ws);
  return s.substr(a, b - a + 1);
}

bool ConfigFile::ExtractKeys() {  // config_file.cpp:76-104
  std::ifstream file(fName_.c_str());
  if (!file) {
    std::cout << "Config file " + fName_ + " could not be found!\n";
    return false;
  }
  std::string line;
  size_t lineNo = 0;
  while (std::getline(file, line)) {
    lineNo++;
    size_t hash = line.find('#');
    if (hash != std::string::npos) line.erase(hash);
    if (trim(line).empty()) continue;
    size_t eq = line.find('=');
    if (eq == std::string::npos) {
      std::cout << "CFG: Bad format for line: " << lineNo << "\n";
      continue;
    }
    std::string key = trim(line.substr(0, eq)), val = trim(line.substr(eq + 1));
    if (key.empty()) {
      std::cout << "CFG: Bad format for line: " << lineNo << "\n";
      continue;
    }
    if (!keyExists(key)) contents_[key] = val;  // first definition wins, as the reference's map insert
  }
  return true;
}

std::string ConfigFile::getValueOfKeyAsString(const std::string &key, const std::string &defaultValue) const {
  auto it = contents_.find(key);
  return it == contents_.end() ? defaultValue : it->second;
}
std::vector<double> ConfigFile::getValueOfKeyAsStdVectorDouble(const std::string &key, const std::string &defaultValue) const {
  std::stringstream ss(getValueOfKeyAsString(key, defaultValue));
  std::vector<double> v;
  double x;
  while (ss >> x) v.push_back(x);
  return v;
}
std::vector<int> ConfigFile::getValueOfKeyAsStdVectorInt(const std::string &key, const std::string &defaultValue) const {
  std::stringstream ss(getValueOfKeyAsString(key, defaultValue));
  std::vector<int> v;
  double x;  // the reference parses ints through a double as well (config_file.cpp:154-167)
  while (ss >> x) v.push_back((int)x);
  return v;
}

}  // namespace util
}  // namespace gpd
