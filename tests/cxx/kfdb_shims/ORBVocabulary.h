// ORBVocabulary.h -- repo-authored minimal vocabulary for the KeyFrameDatabase adapter tests: the two members the adapter's
// constructor reads (TemplatedVocabulary::size() and getScoringType(), Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h), and
// the BowVector type (Thirdparty/DBoW2/DBoW2/BowVector.h: a std::map<WordId, WordValue>).
#pragma once
#include <map>

namespace DBoW2 {
typedef unsigned int WordId;
typedef double WordValue;
class BowVector : public std::map<WordId, WordValue> {};
enum ScoringType { L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT };
}

namespace ORB_SLAM2 {
class ORBVocabulary {
public:
    ORBVocabulary(unsigned int nwords, DBoW2::ScoringType scoring) : m_words(nwords), m_scoring(scoring) {}
    unsigned int size() const { return m_words; }
    DBoW2::ScoringType getScoringType() const { return m_scoring; }

private:
    unsigned int m_words;
    DBoW2::ScoringType m_scoring;
};
}
