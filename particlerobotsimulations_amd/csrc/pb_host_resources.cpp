// pb_host_resources.cpp -- the host resources of a rank (include/particlebot_ensemble.h "host resources"): the cores the
// process may really use (hardware, affinity mask, cgroup quota), its share of them among the ranks of the node, the
// cores next to its GPU, and the two clocks the ensemble's accounting reads.
#include <sched.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <string>
#include <thread>
#include <vector>

#include "pb_ensemble.hpp"

namespace {

std::string envOr(const char *name, const char *fallback) {
  const char *v = getenv(name);
  return v && v[0] ? v : fallback;
}

bool readLine(const std::string &path, std::string &out) {
  FILE *f = fopen(path.c_str(), "r");
  if (!f) return false;
  char buf[4096];
  const bool ok = fgets(buf, sizeof buf, f) != nullptr;
  fclose(f);
  if (!ok) return false;
  out = buf;
  while (!out.empty() && (out.back() == '\n' || out.back() == ' ')) out.pop_back();
  return true;
}

// CPUs the cgroup CPU controller grants: the tightest quota / period on the way from the process's own cgroup up to
// the mount point (v2: cpu.max "quota period" or "max period"; v1: cpu.cfs_quota_us, -1 = unlimited).  <= 0: unlimited.
double cgroupCpus() {
  const std::string root = envOr("PB_CGROUP_ROOT", "/sys/fs/cgroup");
  double best = 0.0;
  auto take = [&](double cpus) {
    if (cpus > 0.0 && (best <= 0.0 || cpus < best)) best = cpus;
  };
  // the process's cgroup path: "0::/a/b" (v2) -- inside a container's cgroup namespace this is "/"
  std::string rel = "/";
  if (FILE *f = fopen(envOr("PB_PROC_SELF_CGROUP", "/proc/self/cgroup").c_str(), "r")) {
    char buf[4096];
    while (fgets(buf, sizeof buf, f)) {
      if (strncmp(buf, "0::", 3) == 0) {
        rel = buf + 3;
        while (!rel.empty() && (rel.back() == '\n' || rel.back() == ' ')) rel.pop_back();
        break;
      }
    }
    fclose(f);
  }
  if (rel.empty() || rel[0] != '/' || rel.find("..") != std::string::npos) rel = "/";
  for (std::string dir = rel;;) {
    std::string line;
    if (readLine(root + dir + (dir.back() == '/' ? "" : "/") + "cpu.max", line)) {
      char q[64] = {0};
      double period = 0.0;
      if (sscanf(line.c_str(), "%63s %lf", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0.0) take(atof(q) / period);
    }
    if (dir == "/" || dir.empty()) break;
    const size_t cut = dir.find_last_of('/');
    dir = cut == 0 ? "/" : dir.substr(0, cut);
  }
  std::string q, per;  // cgroup v1
  if (readLine(root + "/cpu/cpu.cfs_quota_us", q) && readLine(root + "/cpu/cpu.cfs_period_us", per) && atof(q.c_str()) > 0 &&
      atof(per.c_str()) > 0)
    take(atof(q.c_str()) / atof(per.c_str()));
  return best;
}

int affinityCpus(cpu_set_t *setOut) {
  cpu_set_t set;
  CPU_ZERO(&set);
  if (sched_getaffinity(0, sizeof set, &set) != 0) return 0;
  if (setOut) *setOut = set;
  return CPU_COUNT(&set);
}

int localWorldSize() {
  for (const char *name : {"LOCAL_WORLD_SIZE", "OMPI_COMM_WORLD_LOCAL_SIZE", "SLURM_NTASKS_PER_NODE"})
    if (const char *v = getenv(name)) return std::max(1, atoi(v));
  return 1;
}

// "0-3,8,10-11" -> the listed cores that are also in the affinity mask
std::vector<int> parseCpuList(const char *text) {
  std::vector<int> cpus;
  cpu_set_t aff;
  const bool haveAff = affinityCpus(&aff) > 0;
  for (const char *p = text; p && *p;) {
    while (*p == ',' || *p == ' ' || *p == '\n') p++;
    if (!*p) break;
    char *end = nullptr;
    const long a = strtol(p, &end, 10);
    if (end == p) break;
    long b = a;
    p = end;
    if (*p == '-') {
      b = strtol(p + 1, &end, 10);
      if (end == p + 1) break;
      p = end;
    }
    for (long c = a; c <= b && c < CPU_SETSIZE; c++)
      if (c >= 0 && (!haveAff || CPU_ISSET((int)c, &aff))) cpus.push_back((int)c);
  }
  return cpus;
}


}  // namespace

// the cores next to a device: /sys/bus/pci/devices/<bus id>/numa_node (>= 0 on a NUMA machine) + local_cpulist
int numaOfDevice(int device, std::string &busId, std::vector<int> &cpus) {
  cpus.clear();
  busId.clear();
  if (device < 0) return -1;
  char id[32] = {0};
  if (const char *fake = getenv("PB_FAKE_PCI_BUS_ID")) {  // CPU tests: no device to ask
    snprintf(id, sizeof id, "%s", fake);
  } else if (pbDevicePciBusId(device, id, (int)sizeof id) != PB_OK) {
    return -1;
  }
  for (char *c = id; *c; c++) *c = (char)tolower(*c);
  busId = id;
  const std::string dir = envOr("PB_SYSFS_ROOT", "/sys") + "/bus/pci/devices/" + busId;
  std::string node, list;
  if (!readLine(dir + "/numa_node", node)) return -1;
  const int n = atoi(node.c_str());
  if (n < 0) return -1;
  if (readLine(dir + "/local_cpulist", list)) cpus = parseCpuList(list.c_str());
  return n;
}

void describeResources(pbHostResources &r, int wanted) {
  memset(&r, 0, sizeof r);
  r.hardware_threads = (int)std::thread::hardware_concurrency();
  r.affinity_cpus = affinityCpus(nullptr);
  r.cgroup_cpus = cgroupCpus();
  int usable = r.hardware_threads > 0 ? r.hardware_threads : 1;
  if (r.affinity_cpus > 0) usable = std::min(usable, r.affinity_cpus);
  if (r.cgroup_cpus > 0.0) usable = std::min(usable, std::max(1, (int)std::floor(r.cgroup_cpus + 1e-9)));
  r.usable_cpus = std::max(1, usable);
  r.local_world_size = localWorldSize();
  int share = std::max(1, r.usable_cpus / r.local_world_size);
  const char *why = "usable cores / ranks of the node";
  bool automatic = true;  // the share is the rule's, not a number somebody asked for
  if (const char *v = getenv("PB_HOST_THREADS")) {
    if (atoi(v) > 0) {
      share = atoi(v);
      why = "PB_HOST_THREADS";
      automatic = false;
    }
  }
  if (wanted > 0) {
    share = wanted;
    why = "host_threads argument";
    automatic = false;
  }
  r.host_threads = std::max(1, std::min(share, 128));
  r.device = -1;
  r.numa_node = -1;
  int dev = -1;
  if (getenv("PB_FAKE_PCI_BUS_ID")) dev = 0;
  else if (pbGetDevice(&dev) != PB_OK) dev = -1;
  r.device = dev;
  std::string bus;
  std::vector<int> cpus;
  r.numa_node = numaOfDevice(dev, bus, cpus);
  snprintf(r.pci_bus_id, sizeof r.pci_bus_id, "%s", bus.c_str());
  r.numa_cpus = (int)cpus.size();
  const char *pin = getenv("PB_PIN_PRODUCERS");
  r.pin_producers = (r.numa_node >= 0 && r.numa_cpus > 0 && !(pin && pin[0] == '0')) ? 1 : 0;
  // A pinned pool must FIT the node's cores: pinning 127 producers of a lone rank to the 64 (NPS4: 16) cores next to
  // its GPU would oversubscribe them 2-8 x while the rest of the machine idles.  Several ranks per node: the cores
  // beyond the node belong to the other ranks' pools, so the automatic share shrinks to the node; a lone rank, or an
  // explicit thread count, keeps its threads and is not pinned.
  const char *pinNote = r.pin_producers ? "pinned to the GPU's NUMA node" : "not pinned (no NUMA node reported for the device)";
  if (pin && pin[0] == '0' && r.numa_node >= 0) pinNote = "not pinned (PB_PIN_PRODUCERS=0)";
  if (r.pin_producers && r.host_threads > r.numa_cpus) {
    if (automatic && r.local_world_size > 1) {
      r.host_threads = r.numa_cpus;
      pinNote = "pinned to the GPU's NUMA node, share clamped to its cores";
    } else {
      r.pin_producers = 0;
      pinNote = "not pinned (the pool is larger than the GPU's NUMA node)";
    }
  }
  char quota[48];
  if (r.cgroup_cpus > 0.0) snprintf(quota, sizeof quota, "%.2f", r.cgroup_cpus);
  else snprintf(quota, sizeof quota, "none");
  snprintf(r.rule, sizeof r.rule,
           "%d producer threads (%s): min(hardware %d, affinity %d, cgroup quota %s) = %d usable / %d rank(s) per node; "
           "%s",
           r.host_threads, why, r.hardware_threads, r.affinity_cpus, quota, r.usable_cpus, r.local_world_size,
           pinNote);
}

// host threads for placement: this rank's share of the cores the process may really use
unsigned hostThreads(int wanted) {
  pbHostResources r;
  describeResources(r, wanted);
  return (unsigned)r.host_threads;
}

double threadCpuSeconds() {
  timespec ts;
  if (clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts) != 0) return 0.0;
  return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

double nowSeconds() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

extern "C" {

int pbHostGetResources(pbHostResources *out) {
  if (!out) return 1;
  describeResources(*out, 0);
  return 0;
}

int pbHostParseCpuList(const char *text, int *cpus, int cap) {
  const std::vector<int> v = parseCpuList(text);
  for (int i = 0; cpus && i < cap && i < (int)v.size(); i++) cpus[i] = v[i];
  return (int)v.size();
}

}  // extern "C"
