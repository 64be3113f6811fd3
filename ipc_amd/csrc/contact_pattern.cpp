#include "contact_pattern.h"
#include <algorithm>
#include <iterator>

namespace ipcgpu {

NodePairs nonMeshPairs(const NodePairs& pairs, const int* nbPtr, const int* nb)
{
    NodePairs out;
    out.reserve(pairs.size());
    for (const auto& e : pairs)
        if (!std::binary_search(nb + nbPtr[e.first], nb + nbPtr[e.first + 1], e.second)) out.push_back(e);
    if (!std::is_sorted(out.begin(), out.end())) std::sort(out.begin(), out.end()); // (the look-ahead list arrives sorted from the device)
    out.erase(std::unique(out.begin(), out.end()), out.end());
    return out;
}

bool ContactPattern::grow(const NodePairs* live, const std::function<NodePairs()>& lookAhead)
{
    if (live && std::includes(pairs_.begin(), pairs_.end(), live->begin(), live->end())) return false;
    // every list here is sorted and unique: a union is one linear merge
    const NodePairs ahead = lookAhead();
    NodePairs padded, merged;
    if (live) std::set_union(live->begin(), live->end(), ahead.begin(), ahead.end(), std::back_inserter(padded));
    else padded = ahead;
    std::set_union(pairs_.begin(), pairs_.end(), padded.begin(), padded.end(), std::back_inserter(merged));
    if (merged.size() > 3 * padded.size() + 4096) merged.swap(padded);
    pairs_.swap(merged);
    flat_.clear();
    flat_.reserve(2 * pairs_.size());
    for (const auto& e : pairs_) flat_.insert(flat_.end(), { e.first, e.second });
    return true;
}

} // namespace ipcgpu
