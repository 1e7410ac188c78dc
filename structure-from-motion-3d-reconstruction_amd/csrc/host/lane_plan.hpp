// lane_plan.hpp -- the order in which the streams of the pipeline's helper contexts are created.  Pure host code: no HIP
// include, no library call, so that a stand-alone program can test it.
//
// The HIP runtime opens a new hardware queue for every stream until GPU_MAX_HW_QUEUES exist, and afterwards gives a stream the
// queue with the fewest streams on it; among equally loaded queues it takes the one at the lowest address, which on the
// machines measured is the one opened last (read from the runtime's own queue log, profiles/lane_plan_ab.txt).  So with nothing
// destroyed in between, creation order is placement, and streams of one queue run their kernels one after the other.  The
// caller's context exists before the pipeline starts, as a (copy, compute) pair, after whatever streams the process made
// before it (`prior`: one in a process that has used the default stream, as under PyTorch).  A plan lists what follows, one
// stream at a time, so that the compute streams of different contexts can be interleaved.  The rule is what the runtime was
// seen to do, not a contract of HIP: the groups stated for the named plans below are the ones the runtime's log showed in the
// benchmark's process (profiles/lane_plan_ab.txt), and tests/lane_plan_main.cpp replays the rule as a model to keep the orders
// and the stated groups consistent.  A process with another number of earlier streams (the CLI has none) gets other groups.
#pragma once

#include <cstdlib>
#include <string>
#include <vector>

namespace sfmx_host {
namespace lane_plan {

// One entry per helper context of a 640x480 run.  P2 is the second prefetch worker's context (pool role PREFETCH, like P).
enum Role { P = 0, T, B, C, A, E, P2, A2, E2, kRoles };
enum Kind { COMPUTE = 0, COPY = 1 };  // the values of sfmx_ctx_create_stream's `which`
struct Step {
  int role, kind;
  bool operator==(const Step& o) const { return role == o.role && kind == o.kind; }
};
struct Plan {
  std::string name;        // a named plan, or "custom" for a spelled-out order
  bool is_default = true;  // chosen by the queue count, not by SFMX_LANE_PLAN
  std::vector<Step> warm;  // created at warm-up, in this order
  std::vector<int> lazy;   // roles left to first use (each then a (copy, compute) pair), in the order a run first uses them
  std::string message;     // why the override was rejected (the default is then in effect); empty otherwise
};

inline const char* role_name(int r) {
  static const char* const n[kRoles] = {"P", "T", "B", "C", "A", "E", "P2", "A2", "E2"};
  return r >= 0 && r < kRoles ? n[r] : "?";
}

// The orders with a name.  A compute stream is written ROLE+, a copy stream ROLE-.  The groups are the compute streams that share
// a queue at four queues in a process with one prior stream (G is the caller's compute stream); idle copy streams fill the rest.
//   parent   (copy, compute) pairs in the order T B P C A E, the rest on first use: the order of every count but four.
//            At four queues: {T, P, A, P2, E2}, {B, C, E, A2}, {G}, and a queue of copy streams.
//   as8      {G, C, A2}, {T, A, E2}, {B, E}, {P, P2}: the default at four queues.  Every queue has compute streams, the BA lane,
//            whose chain of short launches bounds a pass, shares with one edge lane only, the tracker's copy stream is beside
//            the tracker
//   b_own    {B}, {T, P, P2, C}, {G, A, A2, E, E2}: the BA lane beside idle copy streams only; the fourth queue has the default
//            stream and copy streams
//   b_alone  {B}, {T, G}, {P, P2, C}, {A, A2, E, E2}
//   crit     {B, G}, {T}, {P, P2, C}, {A, A2, E, E2}
struct Named { const char* name; const char* order; };
inline const std::vector<Named>& named_plans() {
  static const std::vector<Named> v = {
      {"parent", "T- T+ B- B+ P- P+ C- C+ A- A+ E- E+"},
      {"b_own", "T+ P+ A+ B+ T- P2+ A2+ B- C- C+ E+ A- E- P- E2+ A2- E2- P2-"},
      {"as8", "T+ A+ C+ B+ P+ E2+ A2+ E+ P2+ T- C- B- P- A- A2- E- P2- E2-"},
      {"b_alone", "A+ A2+ T+ B+ P+ E+ T- B- P2+ E2+ C- A- C+ E- A2- E2- P- P2-"},
      {"crit", "A+ A2+ B+ T+ P+ E+ B- T- P2+ E2+ C- A- C+ E- A2- E2- P- P2-"},
  };
  return v;
}
inline const char* default_name(int queue_count) { return queue_count == 4 ? "as8" : "parent"; }

// "T+ B+, P-": tokens separated by blanks or commas.  Every stream at most once, both streams of a role or neither.
inline bool parse(const std::string& s, std::vector<Step>& out, std::string& err) {
  out.clear();
  bool seen[kRoles][2] = {};
  size_t i = 0;
  while (i < s.size()) {
    if (s[i] == ' ' || s[i] == ',' || s[i] == '\t') { ++i; continue; }
    size_t j = i;
    while (j < s.size() && s[j] != ' ' && s[j] != ',' && s[j] != '\t') ++j;
    const std::string tok = s.substr(i, j - i);
    i = j;
    const char k = tok.back();
    if (tok.size() < 2 || (k != '+' && k != '-')) { err = "'" + tok + "' is not ROLE+ (compute) or ROLE- (copy)"; return false; }
    const std::string rn = tok.substr(0, tok.size() - 1);
    int role = -1;
    for (int r = 0; r < kRoles; ++r)
      if (rn == role_name(r)) role = r;
    if (role < 0) { err = "unknown role '" + rn + "' (P T B C A E P2 A2 E2)"; return false; }
    const int kind = k == '+' ? COMPUTE : COPY;
    if (seen[role][kind]) { err = "'" + tok + "' occurs twice"; return false; }
    seen[role][kind] = true;
    out.push_back({role, kind});
  }
  if (out.empty()) { err = "no stream in it"; return false; }
  for (int r = 0; r < kRoles; ++r)
    if (seen[r][COMPUTE] != seen[r][COPY]) { err = std::string("role ") + role_name(r) + " has one of its two streams only"; return false; }
  return true;
}

inline std::string spell(const std::vector<Step>& steps) {
  std::string s;
  for (const Step& st : steps) {
    if (!s.empty()) s += ' ';
    s += role_name(st.role);
    s += st.kind == COMPUTE ? '+' : '-';
  }
  return s;
}

inline void fill_lazy(Plan& p) {
  p.lazy.clear();
  // first use in a run: the prefetch workers, then lanes A/A2, the tracker, and lanes B, C, E, E2
  for (int r : {P, P2, A, A2, T, B, C, E, E2}) {
    bool in = false;
    for (const Step& st : p.warm) in = in || st.role == r;
    if (!in) p.lazy.push_back(r);
  }
}

inline bool named(const std::string& name, Plan& p) {
  for (const Named& n : named_plans())
    if (name == n.name) {
      std::string err;
      p.name = name;
      (void)parse(n.order, p.warm, err);
      fill_lazy(p);
      return true;
    }
  return false;
}

// GPU_MAX_HW_QUEUES as the runtime reads it: unset (or not a positive number) means its default of four.
inline int queue_count(const char* env_value) {
  if (!env_value || !*env_value) return 4;
  char* end = nullptr;
  const long v = std::strtol(env_value, &end, 10);
  return (*end == '\0' && v >= 1 && v <= 1024) ? (int)v : 4;
}

// The plan for `queues` hardware queues.  override_str = SFMX_LANE_PLAN: null for none, a plan's name, or a spelled-out order.
inline Plan choose(int queues, const char* override_str) {
  Plan p;
  if (override_str) {
    const std::string o(override_str);
    std::string err;
    if (named(o, p)) { p.is_default = false; return p; }
    if (o.find_first_not_of(" ,\t") == std::string::npos) err = "it is empty";
    if (err.empty() && parse(o, p.warm, err)) {
      p.name = "custom";
      p.is_default = false;
      fill_lazy(p);
      return p;
    }
    p = Plan();
    p.message = "SFMX_LANE_PLAN='" + o + "' rejected: " + err + "; using the default";
  }
  (void)named(default_name(queues), p);
  return p;
}

// one line: "as8 (default) queues=4 order=T+ A+ ... first_use=-"
inline std::string describe(const Plan& p, int queues) {
  std::string s = p.name + (p.is_default ? " (default)" : " (override)") + " queues=" + std::to_string(queues) + " order=" + spell(p.warm) + " first_use=";
  if (p.lazy.empty()) s += '-';
  for (size_t i = 0; i < p.lazy.size(); ++i) s += (i ? "," : "") + std::string(role_name(p.lazy[i]));
  return s;
}

}  // namespace lane_plan
}  // namespace sfmx_host
