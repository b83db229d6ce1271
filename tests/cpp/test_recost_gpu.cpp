// test_recost_gpu.cpp — LP_gpu<FMC>::upload_costs: the README quick-start model re-solved with other costs on the plan of the first
// solve, cold and warm.  Prints the bounds before and after; tests/test_recost_cpp.py compares them with the Python mirror's, exactly.
// --host-only: compile and link check, nothing runs on a device.
#include <cstdio>
#include <cstring>

#include "LP_gpu.hxx"

using namespace LP_MP_gpu;

struct FMC_SRMP {
  using UnaryFactor = FactorContainer<UnarySimplexFactor, FMC_SRMP, 0, true>;
  using PairwiseFactor = FactorContainer<PairwiseSimplexFactor, FMC_SRMP, 1>;
  using MessageLeft = MessageContainer<UnaryPairwiseMessage<Chirality::left>, 0, 1, message_passing_schedule::left, variableMessageNumber, 1, FMC_SRMP, 0>;
  using MessageRight = MessageContainer<UnaryPairwiseMessage<Chirality::right>, 0, 1, message_passing_schedule::left, variableMessageNumber, 1, FMC_SRMP, 1>;
  using FactorList = meta::list<UnaryFactor, PairwiseFactor>;
  using MessageList = meta::list<MessageLeft, MessageRight>;
};

static void set_table(PairwiseSimplexFactor& p, double a, double b, double c, double d) { p.cost(0, 0) = a; p.cost(0, 1) = b; p.cost(1, 0) = c; p.cost(1, 1) = d; }

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--host-only") == 0) { std::puts("all tests passed (host only: nothing to run)"); return 0; }
  try {
    LP_gpu<FMC_SRMP> lp;
    auto* u1 = lp.add_factor<FMC_SRMP::UnaryFactor>(std::vector<REAL>{0.0, 1.0});
    auto* u2 = lp.add_factor<FMC_SRMP::UnaryFactor>(std::vector<REAL>{1.0, 0.0});
    auto* p = lp.add_factor<FMC_SRMP::PairwiseFactor>(2, 2);
    set_table(*p->GetFactor(), 0.0, 1.0, 1.0, 0.0);
    lp.add_message<FMC_SRMP::MessageLeft>(u1, p);
    lp.add_message<FMC_SRMP::MessageRight>(u2, p);
    lp.AddFactorRelation(u1, p);
    lp.AddFactorRelation(p, u2);
    lp.Begin();
    lp.set_reparametrization(LPReparametrizationMode::Anisotropic);
    std::printf("bound %.17g\n", lp.LowerBound());
    for (INDEX i = 0; i < 3; ++i) lp.ComputePass(i);
    std::printf("bound %.17g\n", lp.LowerBound());
    const int64_t built = lp.schedules_built();
    if (built <= 0) throw std::runtime_error("no schedule was built by three passes");
    // cold: other costs, a fresh problem on the same plan
    (*u1->GetFactor())[0] = 0.7; (*u1->GetFactor())[1] = 0.1;
    set_table(*p->GetFactor(), 0.0, 0.3, 0.6, 0.0);
    lp.upload_costs();
    std::printf("bound %.17g\n", lp.LowerBound());
    for (INDEX i = 0; i < 3; ++i) lp.ComputePass(i);
    std::printf("bound %.17g\n", lp.LowerBound());
    // warm: the messages stay, the changed unary receives new - old
    (*u2->GetFactor())[0] = 0.25; (*u2->GetFactor())[1] = 0.5;
    set_table(*p->GetFactor(), 0.0, 2.0, 2.0, 0.0);
    lp.upload_costs(true);
    std::printf("bound %.17g\n", lp.LowerBound());
    for (INDEX i = 0; i < 2; ++i) lp.ComputePass(i);
    std::printf("bound %.17g\n", lp.LowerBound());
    if (lp.schedules_built() != built) throw std::runtime_error("upload_costs planned a schedule");
    lp.End();
    std::printf("u2 %.17g %.17g\n", (*u2->GetFactor())[0], (*u2->GetFactor())[1]);
    std::puts("all tests passed");
    return 0;
  } catch (const std::exception& e) {
    std::printf("FAILED: %s\n", e.what());
    return 1;
  }
}
