// Stand-alone driver of csrc/host/lane_plan.hpp for tests/test_lane_plan_cpu.py (host compiler only, no GPU, no library).
//   lane_plan_main plan <queues> [override]     name / default-or-override / warm-up order / first-use roles / message
//   lane_plan_main classes <queues> <override> <prior>  queue of every stream of a full run after <prior> earlier streams: "G- 1", "G+ 2", ...
//   lane_plan_main names                        the named plans
//   lane_plan_main queues [value]               the queue count read from a GPU_MAX_HW_QUEUES value (no value = unset)
// An override given as the word NONE means "SFMX_LANE_PLAN unset"; an empty argument is the empty string.
#include "lane_plan.hpp"

#include <cstdio>
#include <cstring>

namespace lp = sfmx_host::lane_plan;

// A MODEL of the runtime's placement, as its queue log showed it (lane_plan.hpp, top): hardware queue (numbered in the order the
// runtime opens them) of every stream of a full run: `prior`
// streams of the process, the caller's pair, the warm-up order, then the first-use pairs.  out[role][kind]; the caller's own
// streams come back in g_class[kind].
static void classes(const lp::Plan& p, int queues, int prior, int out[lp::kRoles][2], int g_class[2]) {
  std::vector<int> load;
  auto place = [&]() {
    if ((int)load.size() < queues) { load.push_back(1); return (int)load.size() - 1; }
    int best = 0;
    for (int q = 1; q < (int)load.size(); ++q)
      if (load[q] <= load[best]) best = q;  // ties: the queue opened last
    ++load[best];
    return best;
  };
  for (int i = 0; i < prior; ++i) (void)place();
  g_class[lp::COPY] = place();
  g_class[lp::COMPUTE] = place();
  for (const lp::Step& st : p.warm) out[st.role][st.kind] = place();
  for (int r : p.lazy) {
    out[r][lp::COPY] = place();
    out[r][lp::COMPUTE] = place();
  }
}


int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string cmd = argv[1];
  if (cmd == "names") {
    for (const lp::Named& n : lp::named_plans()) std::printf("%s\n", n.name);
    return 0;
  }
  if (cmd == "queues") {
    std::printf("%d\n", lp::queue_count(argc > 2 ? argv[2] : nullptr));
    return 0;
  }
  if (cmd == "sweep") {  // every count 1..32 x (default + every named plan): "<queues> <asked> <name> | <order> | <first use>"
    for (int q = 1; q <= 32; ++q) {
      std::vector<const char*> asked = {nullptr};
      for (const lp::Named& n : lp::named_plans()) asked.push_back(n.name);
      for (const char* a : asked) {
        const lp::Plan p = lp::choose(q, a);
        std::printf("%d %s %s | %s |", q, a ? a : "NONE", p.name.c_str(), lp::spell(p.warm).c_str());
        for (int r : p.lazy) std::printf(" %s", lp::role_name(r));
        std::printf("\n");
      }
    }
    return 0;
  }
  if (argc < 3) return 2;
  const int queues = std::atoi(argv[2]);
  const char* ov = (argc > 3 && std::strcmp(argv[3], "NONE") != 0) ? argv[3] : nullptr;
  const lp::Plan p = lp::choose(queues, ov);
  if (cmd == "plan") {
    std::printf("name=%s\ndefault=%d\norder=%s\nfirst_use=", p.name.c_str(), p.is_default ? 1 : 0, lp::spell(p.warm).c_str());
    for (size_t i = 0; i < p.lazy.size(); ++i) std::printf("%s%s", i ? " " : "", lp::role_name(p.lazy[i]));
    std::printf("\nmessage=%s\ndescribe=%s\n", p.message.c_str(), lp::describe(p, queues).c_str());
    return 0;
  }
  if (cmd == "classes") {
    int cls[lp::kRoles][2], g[2];
    for (auto& c : cls) c[0] = c[1] = -1;
    classes(p, queues < 1 ? 1 : queues, argc > 4 ? std::atoi(argv[4]) : 0, cls, g);
    std::printf("G- %d\nG+ %d\n", g[lp::COPY], g[lp::COMPUTE]);
    for (int r = 0; r < lp::kRoles; ++r) std::printf("%s+ %d\n%s- %d\n", lp::role_name(r), cls[r][lp::COMPUTE], lp::role_name(r), cls[r][lp::COPY]);
    return 0;
  }
  return 2;
}
