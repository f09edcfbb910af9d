// Probabilities, correspondence costs and the 15-bit grid values that stand for them: the reference's
// mapping/probability_values.{h,cc}, once, for host and device code.
//
// Grid contents and scores are compared with the reference bit for bit, so every expression here keeps the
// reference's form and its float type: the scale is (upper - lower) / 32766.f, the offset is lower - scale, and the
// encoder multiplies by 32766.f / (upper - lower).  Do not "simplify" any of them -- (kMax - kMin) / 32766.f and
// 1 / (32766.f / (kMax - kMin)) are different floats.
//
// The constants are constexpr and therefore usable in kernels; kernels that decode values take the three
// ValueToProbability constants as arguments named k_scale, k_offset and k_unknown.
#ifndef DLIOM_CSRC_PROBABILITY_VALUES_H_
#define DLIOM_CSRC_PROBABILITY_VALUES_H_

#include <cmath>
#include <cstdint>

namespace dliom {

// probability_values.h:64-67
constexpr float kMinProbability = 0.1f;
constexpr float kMaxProbability = 1.f - kMinProbability;
constexpr float kMinCorrespondenceCost = 1.f - kMaxProbability;
constexpr float kMaxCorrespondenceCost = 1.f - kMinProbability;

// SlowValueToBoundedFloat (probability_values.cc:27-36): value 0 is "unknown", a value v in [1, 32767] stands for
// v * scale + (lower - scale).
constexpr float kValueToProbabilityScale = (kMaxProbability - kMinProbability) / 32766.f;  // k_scale
constexpr float kValueToProbabilityOffset = kMinProbability - kValueToProbabilityScale;    // k_offset
constexpr float kUnknownProbability = kMinProbability;                                     // k_unknown
constexpr float kValueToCorrespondenceCostScale = (kMaxCorrespondenceCost - kMinCorrespondenceCost) / 32766.f;
constexpr float kValueToCorrespondenceCostOffset = kMinCorrespondenceCost - kValueToCorrespondenceCostScale;
constexpr float kUnknownCorrespondenceCost = kMaxCorrespondenceCost;

// common::Clamp (common/math.h:32-41)
inline float clampf(float v, float lo, float hi) { return v > hi ? hi : (v < lo ? lo : v); }

// BoundedFloatToValue (probability_values.h:32-44)
inline uint16_t bounded_float_to_value(float f, float lo, float hi) {
  const int v = static_cast<int>(std::lround((clampf(f, lo, hi) - lo) * (32766.f / (hi - lo)))) + 1;
  return static_cast<uint16_t>(v);
}
// ProbabilityToValue, CorrespondenceCostToValue (probability_values.h:84-93)
inline uint16_t probability_to_value(float p) { return bounded_float_to_value(p, kMinProbability, kMaxProbability); }
inline uint16_t correspondence_cost_to_value(float c) {
  return bounded_float_to_value(c, kMinCorrespondenceCost, kMaxCorrespondenceCost);
}

// ValueToProbability, ValueToCorrespondenceCost: the entries of the reference's tables (probability_values.cc:27-63),
// whose upper half -- values that carry the update marker -- repeats the lower.
inline float value_to_probability(unsigned v) {
  v &= 32767u;
  return v == 0u ? kUnknownProbability : v * kValueToProbabilityScale + kValueToProbabilityOffset;
}
inline float value_to_correspondence_cost(unsigned v) {
  v &= 32767u;
  return v == 0u ? kUnknownCorrespondenceCost : v * kValueToCorrespondenceCostScale + kValueToCorrespondenceCostOffset;
}

// Odds, ProbabilityFromOdds (probability_values.h:48-54)
inline float odds_of(float p) { return p / (1.f - p); }
inline float probability_from_odds(float odds) { return odds / (odds + 1.f); }

}  // namespace dliom

#endif  // DLIOM_CSRC_PROBABILITY_VALUES_H_
