// The march of the node-owner kernels over the element layers [ez_begin, ez_end) of a strip: a block of statements that poisson3d_q1n_kernel and
// poisson3d_q1n2_kernel (poisson3d_q1.inl) include once in their bodies, after the constant components of the halo records are in LDS.  In scope at
// that point: the type RawNodes, the plane states SA and SB, ez_begin, ez_end, p, and the kernel's own closures
//     plane_request(z, RawNodes&)    issue the loads of node plane z (planes beyond the mesh re-read the last one)
//     plane_publish(RawNodes, z)     Dirichlet conditions, records of plane z into LDS slot z & 1
//     plane_gather(z, S)             records of plane z -> the staged plane S
//     layer(ez, L, U, RawNodes*)     element layer ez between the staged planes L and U; publishes plane ez + 2 (nullptr: nothing) before its ONE
//                                    barrier and finishes node plane ez (emit_plane)
//     top_plane(odd)                 the mesh's top node plane, from the carried cotangents alone (odd: it is SB's plane, else SA's)
//     flush_store()                  the deferred store of the plane finished last
// (The closed form in z, poisson3d_q1_cf.hip, has a loop of its own: literal LDS slots, publish inside the layer.)
{
    // prologue: planes ez_begin and ez_begin + 1 into LDS (both requested before the first is consumed: one memory latency and one barrier
    // instead of two -- a workgroup of a 128^3 launch marches only ~10 layers), the lower one staged
    RawNodes W;
    {
        RawNodes W0;
        plane_request(ez_begin, W0);
        plane_request(ez_begin + 1, W);
        plane_publish(W0, ez_begin);
        plane_publish(W, ez_begin + 1);
    }
    __syncthreads();
    plane_gather(ez_begin, SA);
    __syncthreads();              // every thread has read plane ez_begin before the first layer publishes plane ez_begin + 2 into its slot
    int ez = ez_begin;
    // two layers per trip with the roles of the two plane states swapped: no state copy at the end of a layer
    // (Static or rotating wave priorities per workgroup, against workgroups falling into lock-step, measured equal: profiles/r2_prio3d.txt.)
#pragma nounroll
    for (; ez + 1 < ez_end; ez += 2) {
        plane_request(ez + 2, W);                 // lands while this layer is computed; published before the layer's barrier
        flush_store();
        plane_gather(ez + 1, SB);
        layer(ez, SA, SB, &W);
        plane_request(ez + 3, W);
        flush_store();
        plane_gather(ez + 2, SA);
        layer(ez + 1, SB, SA, &W);
    }
    bool odd = false;
    if (ez < ez_end) {
        flush_store();
        plane_gather(ez + 1, SB);
        layer(ez, SA, SB, nullptr);
        odd = true;
    }
    flush_store();
    if (ez_end == p.nelz) {       // the last strip owns the top boundary plane: only the layer below contributes
        top_plane(odd);
        flush_store();
    }
}
