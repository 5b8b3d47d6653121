// The element-owner march over the node rows j0 .. j1 - 1 of a strip (q1_owner_march.h has the mapping), written once: a block of
// statements, included in the body of ns2d_kernel, transport2d_kernel and coef_grad2d_kernel.  It is text and not a function on purpose:
// as a forceinline template that received the four closures, ns2d_kernel<2, true, false, false, false> came out with its store guards
// arranged differently (same registers, 3205 instead of 3221 instructions) and ran 0.9 % slower at 2049^2, B = 8; included as text the
// masked kernels have the instruction counts they had with the march spelled out in each file (profiles/owner_march_refactor.txt).
//
// In scope at the point of inclusion:
//     NF                                           outputs per node (3, 1, 2)
//     Raw, Row                                     the raw loads of one node row; a landed row.  prev = cur copies a whole Row, so a Row type
//                                                  gives every member that some form's consume leaves unset a default initialiser
//     j0, j1                                       the strip's node rows
//     issue(r, Raw&)                               the loads of node row r (clamped into the mesh) and of the element layer r - 1 under it
//     consume(const Raw&, Row&)                    a landed row: substitutions, the right neighbours
//     element(prev, cur, W, e, bot, top)           the lane's element in element row e (node rows e, e + 1: prev, cur; W: the raw row e + 1
//                                                  with the element layer e): the parts of its contributions that belong to the lane's node
//                                                  in rows e (bot) and e + 1 (top), zero where the element does not exist; it sets all NF of
//                                                  each, so that the carry never copies an indeterminate value
//     finish(e, prev, carry, bot)                  node row e is complete (carry + bot): Dirichlet rows, sums of squares, the store
{
    Row prev, cur;
    float carry[NF];
#pragma unroll
    for (int k = 0; k < NF; ++k) carry[k] = 0.f;
    // two rows in flight ahead of the element row being computed (W0, W1 alternate; unrolled by two so that no register with a load
    // outstanding is ever copied -- a copy would wait for it)
    Raw W0, W1;
    {
        Raw A;
        issue(j0 - 1, A);
        issue(j0, W0);
        issue(j0 + 1, W1);
        consume(A, prev);
    }
    // element row e (from e = j0 - 1, the halo row): W holds the raw node row e + 1 and the element layer e; refilled with row e + 3.
    // Node row e is finished here.
    auto step = [&](int e, Raw& W) {
        consume(W, cur);
        float bot[NF], top[NF];
        element(prev, cur, W, e, bot, top);
        issue(e + 3, W);
        if (e >= j0) finish(e, prev, carry, bot);
#pragma unroll
        for (int k = 0; k < NF; ++k) carry[k] = top[k];
        prev = cur;
    };
    for (int e = j0 - 1; e < j1; e += 2) {
        step(e, W0);
        if (e + 1 < j1) step(e + 1, W1);
    }
}
