/* ffhip_parts.h -- how a call that answers per item cuts its items into PARTS: the budget a part's weights stay under, the
 * greedy cut, and what a part's return code does to the call's.  Plain C++ with no HIP in it, so that tests/tools/check_parts.cpp runs it
 * on the CPU.  What a part IS -- its weight, its scratch, its launches -- stays with the caller. */
#ifndef FFHIP_PARTS_H
#define FFHIP_PARTS_H

#include "ffpic_hip.h"

#include <limits.h>
#include <stddef.h>
#include <stdlib.h>

/* a *_PART_BYTES switch's value -> a part's budget */
inline size_t ffhip_part_budget(const char *v)
{
    const long long b = v ? atoll(v) : 0;
    return b > 0 ? (size_t)b : (size_t)1 << 30;
}

constexpr int FFHIP_PARTS_NO_CAP = INT_MAX; /* max_items of a call whose records stay small by its budget alone */

/* Items [0, n) in order, part(first, cnt) for each part.  A part takes items while there are fewer than max_items of them and their
 * weight(i) sum to budget at most; an item beyond the budget is a part of its own.  FFHIP_EINVAL, FFHIP_ENOMEM, FFHIP_EIO and FFHIP_ENODEV
 * of a part end the call at once; of the others (the items' verdicts) the first that is not FFHIP_OK is the call's, and the later parts
 * still run */
template <class Weight, class Part> int ffhip_parts_run(int n, size_t budget, int max_items, Weight weight, Part part)
{
    int first_rc = FFHIP_OK;
    for (int first = 0; first < n;) {
        int cnt = 0;
        size_t sum = 0;
        while (first + cnt < n && cnt < max_items) {
            const size_t w = weight(first + cnt);
            if (cnt && sum + w > budget) break;
            sum += w;
            cnt++;
        }
        const int rc = part(first, cnt);
        if (rc == FFHIP_EINVAL || rc == FFHIP_ENOMEM || rc == FFHIP_EIO || rc == FFHIP_ENODEV) return rc;
        if (first_rc == FFHIP_OK) first_rc = rc;
        first += cnt;
    }
    return first_rc;
}

#endif
